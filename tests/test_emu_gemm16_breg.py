"""fd_pw_gemm16_f32's register form of the weight fragments against its LDS form on the CPU emulator (checks and cases: tests/gemm16_breg.py;
the same run on the device in tests/test_gpu_gemm16_breg.py)."""
import pytest

import forms
import gemm16_breg as breg


@pytest.mark.parametrize("name,plan,b,hw", forms.GEMM16_CASES)
def test_emulated_gemm16_register_form_is_bitwise_the_lds_form(name, plan, b, hw):
    breg.check_bitwise_ab("emu", name, plan, b, hw)


@pytest.mark.parametrize("name,b,tile,fused,dw", breg.FUSED_CASES)
def test_emulated_gemm16_register_form_fused_consumer_image(name, b, tile, fused, dw):
    breg.check_fused_consumer_image("emu", name, b, tile, fused, dw)


def test_emulated_gemm16_register_form_short_k():
    breg.check_short_k("emu")


def test_emulated_gemm16_register_form_long_k_branch_free_path():
    breg.check_long_k("emu")


def test_emulated_gemm16_train_forward_ignores_the_form_bit():
    breg.check_train_forward("emu")
