"""CPU-emulated runs of the product's HIP kernels + plan code through the C ABI (tests/hipemu), checked against
the C oracle.  These catch indexing / tiling / barrier / MFMA-layout bugs without a GPU; the same checks and case tables
(tests/forms.py) run on the device in test_gpu_forms.py, the full-size parity tests are the `gpu`-marked ones in test_gpu_parity.py."""
import pytest
import torch

import forms
import harness
from forms import G16, RAGGED, TINY, TOL, UNITS, WIDE, small_model  # noqa: F401  (other test modules import them from here)


@pytest.mark.parametrize("name,plan,b,hw", forms.FORWARD_CASES)
def test_emulated_forward_matches_oracle(name, plan, b, hw):
    forms.check_forward_matches_oracle("emu", name, plan, b, hw)


@pytest.mark.parametrize("name,plan,b,hw", forms.GEMM16_CASES)
def test_emulated_gemm16_matches_oracle(name, plan, b, hw):
    forms.check_gemm16_matches_oracle("emu", name, plan, b, hw)


@pytest.mark.parametrize("b,hw", forms.DWPW_CASES)
def test_emulated_dwpw_units_match_oracle(b, hw):
    forms.check_dwpw_units_match_oracle("emu", b, hw)


def test_plan_rejects_bad_shapes():
    m = small_model(*TINY, seed=1)
    with pytest.raises(harness.capi.FastDepthError):
        harness.CPlan("emu", m, torch.rand(1, 3, 48, 64))       # not a multiple of 32 (reference fails at the skip add)


@pytest.mark.parametrize("dtype,tol", forms.H16_FORWARD_DTYPES)
@pytest.mark.parametrize("name,plan", forms.H16_FORWARD_MODELS)
def test_emulated_16bit_forward_matches_oracle(name, plan, dtype, tol):
    forms.check_16bit_forward_matches_oracle("emu", name, plan, dtype, tol)


def test_emulated_no_skip_sibling_forward():
    forms.check_no_skip_sibling_forward("emu")


def test_emulated_skip_concat_sibling_forward():
    forms.check_skip_concat_sibling_forward("emu")


@pytest.mark.parametrize("dtype,ulp", forms.ULP_DTYPES)
@pytest.mark.parametrize("name,plan,b,hw,flags", forms.H16_GEMM16_CASES)
def test_emulated_16bit_gemm16_and_fused_epilogues(name, plan, b, hw, flags, dtype, ulp):
    forms.check_16bit_gemm16_and_fused_epilogues("emu", name, plan, b, hw, flags, dtype, ulp)


@pytest.mark.parametrize("dtype", forms.H16_DTYPES)
@pytest.mark.parametrize("name,plan", forms.H16_FORWARD_MODELS)
def test_emulated_16bit_head_on_the_last_gemm(name, plan, dtype):
    forms.check_16bit_head_on_the_last_gemm("emu", name, plan, dtype)


@pytest.mark.parametrize("dtype,ulp", forms.ULP_DTYPES)
@pytest.mark.parametrize("b,hw", forms.DW_H8_CASES)
def test_emulated_16bit_depthwise_8_channels_per_work_item(b, hw, dtype, ulp):
    forms.check_16bit_depthwise_8_channels_per_work_item("emu", b, hw, dtype, ulp)


@pytest.mark.parametrize("dtype,ulp", forms.ULP_DTYPES)
@pytest.mark.parametrize("b,hw", forms.DW5_ROWS_CASES)
def test_emulated_16bit_dw5_rows_pixel_pair_kernel(b, hw, dtype, ulp):
    forms.check_16bit_dw5_rows_pixel_pair_kernel("emu", b, hw, dtype, ulp)
