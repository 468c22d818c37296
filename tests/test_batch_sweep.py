"""CPU tier of the batch sweep (tests/batch_sweep.py): the committed batch lists really cover what the default inference plan selects.

Plans are only CREATED here, on the emulator build of the library (the plan code is host code, the same source on both tiers, and its CU
count is a constant): no kernel runs.  When someone moves a threshold of csrc/fd_plan_select.h / csrc/fd_plan_build.h, the coverage test
fails here and names every (layer, form) no listed batch size reaches, with a batch size that does; `python tests/batch_sweep.py` prints
the new lists.  tests/test_gpu_batch_sweep.py runs the listed sizes on the device."""
import functools

import pytest

import batch_sweep as bs


@functools.lru_cache(maxsize=None)
def sweep(config):
    """{B: [(layer, key)]} for B = 1 ... 128: enumerated once per configuration, shared by the tests below"""
    return {b: bs.plan_keys("emu", config, b) for b in bs.SWEEP}


def table_of(per_b):
    table = {}
    for b, pairs in per_b.items():
        for pair in pairs:
            table.setdefault(pair, set()).add(b)
    return table


@pytest.mark.parametrize("config", bs.CONFIGS)
def test_batch_lists_cover_every_selected_form(config):
    table = table_of(sweep(config))
    assert len(table) > 38                                       # more pairs than layers: the selection does move with B
    assert all(table[pair] >= hit for pair, hit in bs.enumerate_forms("emu", config, [16, 128]).items())      # the function the GPU tier calls agrees
    missing = bs.uncovered(table, bs.BATCHES[config])
    assert not missing, "%s: %d (layer, form) pairs of B = 1 ... 128 are reached by no batch size of BATCHES (regenerate: python tests/batch_sweep.py):\n%s" % (
        config, len(missing), "\n".join("  %s: %s   -- first at B = %d" % m for m in missing))


@pytest.mark.parametrize("config", bs.CONFIGS)
def test_batch_lists_are_bounded_and_hold_the_ordinary_sizes(config):
    lst = bs.BATCHES[config]
    assert len(lst) <= bs.MAX_LIST and lst == sorted(set(lst)) and {8, 16} <= set(lst), lst
    assert set(lst) <= set(bs.SWEEP)
    assert len(bs.cover_batches(table_of(sweep(config)))) <= bs.MAX_LIST       # what a regeneration would commit fits too


@pytest.mark.parametrize("config", bs.CONFIGS)
def test_committed_digests_are_the_emulator_tiers_selection(config):
    """FORM_DIGESTS is what the device plan is held to (check_batch): it must be what this tier derives."""
    per_b = sweep(config)
    assert set(bs.FORM_DIGESTS[config]) == set(bs.BATCHES[config])
    stale = {b: (d, bs.digest(per_b[b])) for b, d in bs.FORM_DIGESTS[config].items() if d != bs.digest(per_b[b])}
    assert not stale, "%s: the selection at these batch sizes changed (B: committed, now) -- regenerate with python tests/batch_sweep.py: %s" % (config, stale)


def test_greedy_cover_on_a_hand_made_table():
    table = {("a", "x"): {1, 2, 3}, ("a", "y"): {4}, ("b", "x"): {2, 4}, ("c", "z"): {3, 5}}
    assert bs.cover_batches(table, always=()) == [2, 3, 4]          # 2, 3 and 4 each hit two pairs: the smallest goes first, then one pair per pick
    assert bs.cover_batches(table) == [2, 3, 4, 8, 16]
    assert bs.uncovered(table, [1, 2]) == [("a", "y", 4), ("c", "z", 3)]
    assert bs.coverage_row(table) == (5, 4, 4)


KEY_CASES = [
    ("stem3x3s2<mfma 32x32x2, LDS-staged rows, 256 px per workgroup> grid=49x16 lds=36864",
     "stem3x3s2<mfma 32x32x2, LDS-staged rows, 256 px per workgroup>"),
    ("(fused into layer 2)", "(fused into layer N)"),
    ("dwpw<dw k5 s1 mode2 + pw> persistent, 4 producer + 4 consumer waves; tile 16x8 px x all 32 channels, C=64 in 2 chunks, weights in LDS, grid=256 lds=88576 + the 32->1 head on the accumulators",
     "dwpw<dw k5 s1 mode2 + pw> persistent, 4 producer + 4 consumer waves; tile 16x8 px x all 32 channels, C=64 in 2 chunks, weights in LDS + the 32->1 head on the accumulators"),
    ("dw3_rows8<s1> rows/item 7 grid=1x16x64", "dw3_rows8<s1> rows/item 7"),
    ("dw3_rows<s2> rows/item 14 grid=4x4x64", "dw3_rows<s2> rows/item 14"),
    ("dwconv<k5 s1 mode1> tile 7x16x32 pitch 40 grid=2x16x16 lds=38528, 4 channels per work-item", "dwconv<k5 s1 mode1> tile 7x16x32 pitch 40, 4 channels per work-item"),
    ("dw5_rows<k5 s1 mode2, pixel pairs + dot2, 64 channel lanes per strip> bands of 14 rows, 7 strip groups, 128 channels per block, grid=4x2x64, no LDS",
     "dw5_rows<k5 s1 mode2, pixel pairs + dot2, 64 channel lanes per strip> bands of 14 rows, 7 strip groups, 128 channels per block, no LDS"),
    ("pw_gemm<64x128> M=6272 N=512 K=256 tiles=98x4 lds=73728", "pw_gemm<64x128> N=512 K=256"),
    ("pw_gemm<64x64> M=802816 N=16 K=56 tiles=12544x1 lds=16384 + the 16->1 head on its output tile", "pw_gemm<64x64> N=16 K=56 + the 16->1 head on its output tile"),
    ("pw_gemm16<TM=13: 208x64 tile, stride 196> M=12544 N=256 K=256 tiles=64x4 (1.00 per CU) lds=139264", "pw_gemm16<TM=13: 208x64 tile, stride short/odd> N=256 K=256"),
    ("pw_gemm16<TM=13: 208x64 tile, stride 208> M=13312 N=256 K=256 tiles=64x4 (1.00 per CU) lds=139264", "pw_gemm16<TM=13: 208x64 tile, stride full> N=256 K=256"),
    ("pw_gemm16<TM=7: 112x64 tile, stride 96> M=3072 N=512 K=512 tiles=32x8 (1.00 per CU) lds=57344, weight fragments in registers",
     "pw_gemm16<TM=7: 112x64 tile, stride short/16> N=512 K=512, weight fragments in registers"),
    ("pw_gemm16<TM=4: 64x64 tile, stride 49> M=784 N=1024 K=1024 tiles=16x16 (1.00 per CU) lds=33184, weight fragments in registers + fused dw k5 of layer 27",
     "pw_gemm16<TM=4: 64x64 tile, stride short/odd> N=1024 K=1024, weight fragments in registers + fused dw k5 of layer N"),
    ("(dw k5 s1 on up2 evaluated in the epilogue of layer 28's pw_gemm16)", "(dw k5 s1 on up2 evaluated in the epilogue of layer N's pw_gemm16)"),
    ("(pointwise head evaluated on the accumulators of layer 36's dwpw kernel)", "(pointwise head evaluated on the accumulators of layer N's dwpw kernel)"),
    ("head_pw1 up=1 grid=6272", "head_pw1 up=1"),
]


@pytest.mark.parametrize("line,key", KEY_CASES, ids=[c[0].split("<")[0].split(" ")[0].strip("(") + str(i) for i, c in enumerate(KEY_CASES)])
def test_form_key_of_literal_info_lines(line, key):
    assert bs.form_key(line) == key


def test_form_key_keeps_what_tells_forms_apart():
    base = "pw_gemm16<TM=7: 112x64 tile, stride 98> M=3136 N=512 K=256 tiles=32x8 (1.00 per CU) lds=57344, weight fragments in registers"
    same = "pw_gemm16<TM=7: 112x64 tile, stride 99> M=6336 N=512 K=256 tiles=64x8 (2.00 per CU) lds=57344, weight fragments in registers"
    assert bs.form_key(base) == bs.form_key(same)
    for other in (base.replace("TM=7: 112x64", "TM=4: 64x64"), base.replace("stride 98", "stride 96"), base.replace("stride 98", "stride 112"), base.replace("N=512", "N=256"),
                  base.replace("K=256", "K=512"), base.replace(", weight fragments in registers", ""), base + " + fused dw k3 of layer 25", base.replace("pw_gemm16", "pw_gemm")):
        assert bs.form_key(other) != bs.form_key(base), other
    assert bs.form_key("dw3_rows<s1> rows/item 4 grid=7x14x16") != bs.form_key("dw3_rows<s1> rows/item 14 grid=7x14x16")
    assert bs.form_key("pw_gemm<64x64> M=50176 N=128 K=128 tiles=784x2 lds=49152") != bs.form_key("pw_gemm<128x64> M=50176 N=128 K=128 tiles=392x2 lds=73728")
    assert [bs.stride_class(4, s) for s in (64, 48, 49, 16)] == ["full", "short/16", "short/odd", "short/16"]


def test_pruned_bf16_bound_is_four_times_the_references_own_drift():
    """BOUND_REF['bf16_pruned'] is derived, not a project bound: the committed drift is re-measured (torch_ref in bfloat16 against fp64 on the
    sweep's eight frames; CPU kernels may differ in the last bits between machines, hence a band and not equality)."""
    d = bs.measure_bf16_drift()
    assert bs.BOUND_REF["bf16_pruned"] == 4 * bs.BF16_PRUNED_DRIFT
    assert 0.5 * d <= bs.BF16_PRUNED_DRIFT <= 2 * d, (d, bs.BF16_PRUNED_DRIFT)
    assert [bs.frame_of(n) for n in range(9)] == [3, 0, 5, 2, 7, 4, 1, 6, 3]
