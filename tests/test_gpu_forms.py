"""The small-shape kernel-form matrix of the CPU-emulator tier, on a real MI355X: the same checks, case tables, models, seeds, shapes and
tolerances (tests/forms.py, tests/test_emu_nonfinite.py) with kind = "hip".

The emulator runs one workgroup at a time with one fiber per work-item, so it cannot see races between workgroups (the last-arriver reductions, the
consumer-side BatchNorm finalisation from the integer statistics rows, the leader / follower LDS-DMA ring), barriers that only hardware scheduling
misses, LDS / register limits (its __shared__ is static, its __launch_bounds__ empty), the raw-buffer range check fd_dw5_rows pads with, nor the
hardware side of any FD_EMU branch of csrc/ (DPP, MFMA, packed conversions, v_dot2, the NaN-propagating max / med3 / packed ReLU).  The full-size
device tests (test_gpu_parity.py, test_gpu_train.py) run the default forms at 224 x 224, where none of this matrix's edges occurs: half-empty waves,
ragged last bands and tiles, ragged M / N / K, 1 ... 4 channel chunks, the forced forms of csrc/fd_tuning.h.

The bit-equality assertions (fd_lane<T, 8> layers equal to the 4-channel form, the layers before the first dw5_rows unit, clean frames under poisoned
neighbours) are kept bit-exact on the device.  Run alone: pytest -m gpu tests/test_gpu_forms.py -rA (the FORMS lines are the figures of
profiles/gpu_forms.txt)."""
import pytest

import forms
import test_emu_nonfinite as nonfinite

pytestmark = pytest.mark.gpu


# ---- inference --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,plan,b,hw", forms.FORWARD_CASES)
def test_forward_matches_oracle(name, plan, b, hw):
    forms.check_forward_matches_oracle("hip", name, plan, b, hw)


@pytest.mark.parametrize("name,plan,b,hw", forms.GEMM16_CASES)
def test_gemm16_matches_oracle(name, plan, b, hw):
    forms.check_gemm16_matches_oracle("hip", name, plan, b, hw)


@pytest.mark.parametrize("b,hw", forms.DWPW_CASES)
def test_dwpw_units_match_oracle(b, hw):
    forms.check_dwpw_units_match_oracle("hip", b, hw)


@pytest.mark.parametrize("dtype,tol", forms.H16_FORWARD_DTYPES)
@pytest.mark.parametrize("name,plan", forms.H16_FORWARD_MODELS)
def test_16bit_forward_matches_oracle(name, plan, dtype, tol):
    forms.check_16bit_forward_matches_oracle("hip", name, plan, dtype, tol)


def test_no_skip_sibling_forward():
    forms.check_no_skip_sibling_forward("hip")


def test_skip_concat_sibling_forward():
    forms.check_skip_concat_sibling_forward("hip")


@pytest.mark.parametrize("dtype,ulp", forms.ULP_DTYPES)
@pytest.mark.parametrize("name,plan,b,hw,flags", forms.H16_GEMM16_CASES)
def test_16bit_gemm16_and_fused_epilogues(name, plan, b, hw, flags, dtype, ulp):
    forms.check_16bit_gemm16_and_fused_epilogues("hip", name, plan, b, hw, flags, dtype, ulp)


@pytest.mark.parametrize("dtype", forms.H16_DTYPES)
@pytest.mark.parametrize("name,plan", forms.H16_FORWARD_MODELS)
def test_16bit_head_on_the_last_gemm(name, plan, dtype):
    forms.check_16bit_head_on_the_last_gemm("hip", name, plan, dtype)


@pytest.mark.parametrize("dtype,ulp", forms.ULP_DTYPES)
@pytest.mark.parametrize("b,hw", forms.DW_H8_CASES)
def test_16bit_depthwise_8_channels_per_work_item(b, hw, dtype, ulp):
    forms.check_16bit_depthwise_8_channels_per_work_item("hip", b, hw, dtype, ulp)


@pytest.mark.parametrize("dtype,ulp", forms.ULP_DTYPES)
@pytest.mark.parametrize("b,hw", forms.DW5_ROWS_CASES)
def test_16bit_dw5_rows_pixel_pair_kernel(b, hw, dtype, ulp):
    forms.check_16bit_dw5_rows_pixel_pair_kernel("hip", b, hw, dtype, ulp)


@pytest.mark.parametrize("name,plan,hw,dtype,flags", nonfinite.INFER_CASES, ids=[c[0] for c in nonfinite.INFER_CASES])
def test_forward_propagates_nonfinite_like_reference(name, plan, hw, dtype, flags):
    nonfinite.check_forward_propagates_nonfinite_like_reference("hip", name, plan, hw, dtype, flags)


# ---- train step -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,plan,b", forms.TRAIN_E2E_CASES)
def test_train_forward_backward(name, plan, b):
    forms.check_train_forward_backward("hip", name, plan, b)


@pytest.mark.parametrize("name,plan,dtype,flags", forms.TRAIN_LOCAL_CASES)
def test_train_step_layer_local(name, plan, dtype, flags):
    forms.check_train_step_layer_local("hip", name, plan, dtype, flags)


@pytest.mark.parametrize("dtype", forms.STAT_ROWS_DTYPES)
def test_statistics_rows_cover_large_and_small_magnitudes(dtype):
    forms.check_statistics_rows_cover_large_and_small_magnitudes("hip", dtype)


@pytest.mark.parametrize("dtype,flags", forms.SKIP_CONCAT_TRAIN_CASES)
def test_skip_concat_train_step_layer_local(dtype, flags):
    forms.check_skip_concat_train_step_layer_local("hip", dtype, flags)


@pytest.mark.parametrize("name,dtype,flags", nonfinite.TRAIN_CASES, ids=[c[0] for c in nonfinite.TRAIN_CASES])
def test_train_step_with_nan_pixel_like_reference(name, dtype, flags):
    nonfinite.check_train_step_with_nan_pixel_like_reference("hip", name, dtype, flags)
