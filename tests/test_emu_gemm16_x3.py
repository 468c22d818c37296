"""The split-bf16 form of fd_pw_gemm16_f32 on the CPU emulator (checks and cases: tests/gemm16_x3.py; the same run on the device in
tests/test_gpu_gemm16_x3.py).  The emulator's bf16 MFMA accumulates in its own order: the error bound is what both tiers share."""
import pytest

import gemm16_x3 as x3
import test_emu_nonfinite as nonfinite
from forms import F, RAGGED, TINY


@pytest.mark.parametrize("name,plan,b,hw", x3.PLANE_CASES, ids=[c[0] for c in x3.PLANE_CASES])
def test_emulated_x3_planes_are_exact_splits(name, plan, b, hw):
    x3.check_planes("emu", name, plan, b, hw)


@pytest.mark.parametrize("name,plan,b,hw", x3.CASES, ids=[c[0] for c in x3.CASES])
def test_emulated_x3_gemm_against_fp64(name, plan, b, hw):
    x3.check_gemm_against_fp64("emu", name, plan, b, hw)


def test_emulated_x3_cases_reach_every_path():
    x3.check_case_coverage("emu")


def test_emulated_x3_nonfinite_classes_match_the_fp32_form():
    x3.check_nonfinite_classes("emu")


@pytest.mark.parametrize("name,plan,b,hw", x3.PLANE_CASES, ids=[c[0] for c in x3.PLANE_CASES])
def test_emulated_x3_nonfinite_a_rows_keep_their_class(name, plan, b, hw):
    x3.check_nonfinite_a_rows("emu", name, plan, b, hw)


def test_emulated_x3_default_plan_picks_five_layers_and_agrees_with_the_forced_plan_in_front_of_the_sixth():
    x3.check_default_plan_geometry("emu")


@pytest.mark.parametrize("name,plan,hw", [("tiny_f32_gemm16_x3", TINY, (64, 64)), ("ragged_f32_gemm16_x3_rect", RAGGED, (32, 96))])
def test_emulated_x3_forward_propagates_nonfinite_like_reference(name, plan, hw):
    import torch
    nonfinite.check_forward_propagates_nonfinite_like_reference("emu", name, plan, hw, torch.float32, F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_FORCE_G16_X3)
