"""Edge cases of the service kernels (fd_l1_loss, fd_l1_loss_masked, fd_sgd_step, fd_cast_gradients, fd_depth_metrics, fd_depth_metrics_frames) on a real
MI355X: the checks, case tables, seeds and bounds of tests/service_ref.py with kind = "hip".

The device-only side of these cases: the hardware bf16 conversion behind fd_f32_to_bf16 / fd_f32x2_to_bf16x2 (the emulator tier runs the integer formula
itself), the device's logf / division / contraction in the metrics, misaligned pointers under real 16-byte accesses, and many workgroups in flight over
one scratch buffer.  Run alone: pytest -m gpu tests/test_gpu_service.py -rA (the FORMS lines are the figures of profiles/gpu_service.txt)."""
import pytest

import service_ref as S

pytestmark = pytest.mark.gpu

KIND = "hip"


@pytest.mark.parametrize("numel", S.L1_SIZES)
def test_l1_loss(numel):
    S.check_l1(KIND, False, numel, "plain")


@pytest.mark.parametrize("numel", S.L1_SIZES)
def test_l1_loss_masked(numel):
    S.check_l1(KIND, True, numel, "mixed")


@pytest.mark.parametrize("variant,numel", S.L1_MASKED_SPECIALS)
def test_l1_loss_masked_special_selections(variant, numel):
    S.check_l1(KIND, True, numel, variant)


@pytest.mark.parametrize("masked", [False, True])
def test_l1_loss_scratch_reuse(masked):
    S.check_l1_scratch_reuse(KIND, masked)


@pytest.mark.parametrize("hyper", S.SGD_HYPER, ids=lambda h: "lr%g-m%g-wd%g-gs%g" % h)
@pytest.mark.parametrize("layout,shifts", S.SGD_LAYOUTS)
def test_sgd_step(layout, shifts, hyper):
    S.check_sgd(KIND, layout, shifts, hyper)


def test_sgd_step_against_torch():
    S.check_sgd_against_torch(KIND)


@pytest.mark.parametrize("layout,shifts,tail", S.CAST_VALUE_CASES)
def test_cast_f32_to_bf16_value_set(layout, shifts, tail):
    S.check_cast_to_bf16_values(KIND, layout, shifts, tail)


@pytest.mark.parametrize("layout,shifts,tail", S.CAST_VALUE_CASES)
def test_cast_bf16_to_f32_value_set(layout, shifts, tail):
    S.check_cast_from_bf16_values(KIND, layout, shifts, tail)


@pytest.mark.parametrize("numel,src_shift", S.CAST_SIZE_CASES)
def test_cast_sizes_and_round_trip(numel, src_shift):
    S.check_cast_sizes(KIND, numel, src_shift)


@pytest.mark.parametrize("n_frames,frame_numel,seed", S.METRICS_POOLED)
def test_depth_metrics_pooled(n_frames, frame_numel, seed):
    S.check_metrics_pooled(KIND, n_frames, frame_numel, seed)


@pytest.mark.parametrize("n_frames,frame_numel,seed", S.METRICS_FRAMES)
def test_depth_metrics_frames(n_frames, frame_numel, seed):
    S.check_metrics_frames(KIND, n_frames, frame_numel, seed)


@pytest.mark.parametrize("name", S.METRICS_SPECIALS)
def test_depth_metrics_special_pixels(name):
    S.check_metrics_special(KIND, name)


def test_depth_metrics_all_invalid_frame():
    S.check_metrics_all_invalid_frame(KIND)


def test_depth_metrics_scratch_reuse():
    S.check_metrics_scratch_reuse(KIND)
