"""Plans on poisoned workspaces with guards on every caller buffer, on the CPU emulator: the checks, case tables and assertions of tests/integrity_ref.py with
kind = "emu".  The cases beyond about forty inference plans and a dozen train steps are marked slow; the ones the table keeps for the device tier (full-width
siblings in 16 bits, the 16-bit and further flag sets of UNITS, the 16-bit 224 x 32 train step: minutes each on the emulator, milliseconds on the device) are
not run here -- `slow` cases run with the default suite, so the marker does not bound its time.  The fp32 224 x 32 train step (the only one with a depthwise
map of >= 784 pixels) runs here, marked slow."""
import pytest

import integrity_ref as ref


def _params(cases):
    return [pytest.param(*c[:-1], id=c[0], marks=[pytest.mark.slow] if c[-1] else []) for c in cases if c[-1] is not None]


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.INFER_CASES))
def test_inference_plan_on_poisoned_workspace(cid, model, shape, dtype, flags, keep):
    ref.check_inference_plan("emu", cid, model, shape, dtype, flags, keep)


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.INFER_REUSE_CASES))
def test_inference_plan_reuse(cid, model, shape, dtype, flags, keep):
    ref.check_inference_plan_reuse("emu", cid, model, shape, dtype, flags, keep)


@pytest.mark.parametrize("model,shape,dtype", ref.BUNDLE_CASES, ids=[c[0] for c in ref.BUNDLE_CASES])
def test_bundle_round_trip_on_poisoned_workspace(model, shape, dtype):
    ref.check_bundle_round_trip("emu", model, shape, dtype)


def test_every_kernel_family_writes_a_padded_tensor_or_a_caller_buffer():
    ref.check_family_coverage("emu")


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.TRAIN_CASES))
def test_train_plan_on_poisoned_workspace(cid, model, shape, dtype, flags, keep):
    ref.check_train_plan("emu", cid, model, shape, dtype, flags, keep)


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.TRAIN_REUSE_CASES))
def test_train_plan_reuse(cid, model, shape, dtype, flags, keep):
    ref.check_train_plan_reuse("emu", cid, model, shape, dtype, flags, keep)


def test_every_train_form_runs_next_to_a_padded_tensor():
    ref.check_train_coverage("emu")


def test_pointer_contract_inference():
    ref.check_pointer_contract_inference("emu")


def test_pointer_contract_train():
    ref.check_pointer_contract_train("emu")
