"""The split-bf16 form of fd_pw_gemm16_f32 on the device (checks and cases: tests/gemm16_x3.py; the emulator runs the same in
tests/test_emu_gemm16_x3.py -- but its counted waits are empty and its MFMA is a model: only this tier sees a stage that is read before it has
landed, and the hardware's accumulation order)."""
import pytest
import torch

import gemm16_x3 as x3
import test_emu_nonfinite as nonfinite
from forms import F, RAGGED, TINY

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,plan,b,hw", x3.PLANE_CASES, ids=[c[0] for c in x3.PLANE_CASES])
def test_x3_planes_are_exact_splits(name, plan, b, hw):
    x3.check_planes("hip", name, plan, b, hw)


@pytest.mark.parametrize("name,plan,b,hw", x3.CASES, ids=[c[0] for c in x3.CASES])
def test_x3_gemm_against_fp64(name, plan, b, hw):
    x3.check_gemm_against_fp64("hip", name, plan, b, hw)


def test_x3_nonfinite_classes_match_the_fp32_form():
    x3.check_nonfinite_classes("hip")


@pytest.mark.parametrize("name,plan,b,hw", x3.PLANE_CASES, ids=[c[0] for c in x3.PLANE_CASES])
def test_x3_nonfinite_a_rows_keep_their_class(name, plan, b, hw):
    x3.check_nonfinite_a_rows("hip", name, plan, b, hw)


def test_x3_cases_reach_every_path():
    x3.check_case_coverage("hip")


@pytest.mark.parametrize("name,plan,hw", [("tiny_f32_gemm16_x3", TINY, (64, 64)), ("ragged_f32_gemm16_x3_rect", RAGGED, (32, 96))])
def test_x3_forward_propagates_nonfinite_like_reference(name, plan, hw):
    nonfinite.check_forward_propagates_nonfinite_like_reference("hip", name, plan, hw, torch.float32, F.FD_TUNE_FORCE_GEMM16 | F.FD_TUNE_FORCE_G16_X3)


def test_x3_whole_plan_against_the_oracle():
    x3.check_whole_plan("hip")


def test_x3_default_plan_is_the_forced_plan_where_it_picks_the_form():
    x3.check_default_plan_is_the_forced_plan_where_it_picks_the_form("hip")
