"""The default inference plan (no FD_TUNE_FORCE_* flag, no kept activations -- what the product launches) on a real MI355X at every batch size
of tests/batch_sweep.py's BATCHES: the sizes that between them reach every (layer, kernel form) the plan selects for B = 1 ... 128 at 224 x 224
(tests/test_batch_sweep.py proves the cover on the CPU tier).  224 x 224 is the smallest shape of this test: choose_pw / choose_pw16, the
fusion rules and rows/item are functions of B * 56^2 ... B * 7^2 and of whole frames per tile, so a smaller image reaches other selections.

Per case: the plan's form keys are the enumeration's and the CPU tier's (FORM_DIGESTS), two forwards are bit-equal, and the output is compared
with an fp64 torch_ref run of eight distinct frames (computed once per module) -- fp32: every frame on its own at 1e-3; 16 bit: within 4 ulp
of the first-generation kernels of the same storage type and within the project's bounds of fp64 over the batch (batch_sweep.BOUND_REF).
Run alone: pytest -m gpu tests/test_gpu_batch_sweep.py -rA (one FORMS line per case)."""
import pytest

import batch_sweep as bs

pytestmark = pytest.mark.gpu

CASES = [(config, b) for config in bs.CONFIGS for b in bs.BATCHES[config]]


@pytest.mark.parametrize("config,b", CASES, ids=["%s-B%d" % c for c in CASES])
def test_default_plan_at_batch(config, b):
    bs.check_batch("hip", config, b)
