"""Plans on poisoned workspaces with guards on every caller buffer, on a real MI355X: the checks, case tables and assertions of tests/integrity_ref.py with
kind = "hip" -- the device paths the emulator cannot see (LDS-DMA, packed 16-bit stores, MFMA epilogues, the v_dot2 row walkers, everything under #ifndef FD_EMU).
Run alone: pytest -m gpu tests/test_gpu_integrity.py -rA (the FORMS lines are the figures of profiles/gpu_integrity.txt)."""
import pytest

import integrity_ref as ref

pytestmark = pytest.mark.gpu


def _params(cases):
    return [pytest.param(*c[:-1], id=c[0], marks=[]) for c in cases]


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.INFER_CASES))
def test_inference_plan_on_poisoned_workspace(cid, model, shape, dtype, flags, keep):
    ref.check_inference_plan("hip", cid, model, shape, dtype, flags, keep)


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.INFER_REUSE_CASES))
def test_inference_plan_reuse(cid, model, shape, dtype, flags, keep):
    ref.check_inference_plan_reuse("hip", cid, model, shape, dtype, flags, keep)


@pytest.mark.parametrize("model,shape,dtype", ref.BUNDLE_CASES, ids=[c[0] for c in ref.BUNDLE_CASES])
def test_bundle_round_trip_on_poisoned_workspace(model, shape, dtype):
    ref.check_bundle_round_trip("hip", model, shape, dtype)


def test_every_kernel_family_writes_a_padded_tensor_or_a_caller_buffer():
    ref.check_family_coverage("hip")


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.TRAIN_CASES))
def test_train_plan_on_poisoned_workspace(cid, model, shape, dtype, flags, keep):
    ref.check_train_plan("hip", cid, model, shape, dtype, flags, keep)


@pytest.mark.parametrize("cid,model,shape,dtype,flags,keep", _params(ref.TRAIN_REUSE_CASES))
def test_train_plan_reuse(cid, model, shape, dtype, flags, keep):
    ref.check_train_plan_reuse("hip", cid, model, shape, dtype, flags, keep)


def test_every_train_kernel_runs_next_to_a_padded_tensor_or_writes_a_caller_buffer():
    ref.check_train_coverage("hip")


def test_pointer_contract_inference():
    ref.check_pointer_contract_inference("hip")


def test_pointer_contract_train():
    ref.check_pointer_contract_train("hip")
