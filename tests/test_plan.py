"""The launch plan (authorino_amd/csrc/ajx_plan.h: plan_eval) as a decision table: which
kernel a batch gets and what it is handed, for every live kernel mode, through the host
test library. The expected plans are written out from the rules the plan documents (the
decisions authjx_eval_batch_device used to make inline), not taken from the function."""
import numpy as np
import pytest

import _hosttest as H

EXACT, STREAM, LEAN, TENANT, FUSED, INVALID = range(6)
FULL, STRUCTURAL, NO_FOLD, TIMING = range(4)
MODES = (0, 15, 16, 17, 18, 40, 41, 50, 51, 52, 53)
SHARED_MAX = 48 * 1024  # kMaxSharedBlobBytes
TENANT_MAX = 16 * 1024  # kMaxTenantStageBytes
BIG = 1 << 20


def _in(**kw):
    """One stream-eligible ruleset of 5 selectors (6 stream records), a 3000-byte blob, no
    forest, a bitmap asked for; the default settings."""
    d = dict(n=64, n_sets=1, all_stream=1, max_rec=6, max_sel=5, max_blob=3000, n_trees=0, lean_feat=2, mods=0,
             bitmap=1, force_scan=0, mode=0, len_sort=1, no_tenant_stage=0, stream_max_n=4096)
    d.update(kw)
    return d


def _plan(path, per, **kw):
    """The plan off the stream path of _in()'s ruleset with nothing kept or ordered."""
    d = dict(path=path, stream_mode=FULL, per=per, abl=0, keep_rows=0, rows_stride=6, stage_bytes=0, len_order=0,
             want_pos_of=0, out_k=0, tout_bm=0, n_out=1, lean_feat=2, mods=0)
    d.update(kw)
    return d


ORDERED = dict(len_order=1, want_pos_of=1, out_k=1, tout_bm=1)  # one result per request, in length order
THREE = dict(n_sets=3, max_blob=20000)  # three rulesets, the largest blob over the tenant budget
T3 = dict(lean_feat=3)  # (several rulesets: no walker instance of one ruleset)

TABLE = [
    ("force_scan", _in(force_scan=1), _plan(EXACT, 1)),
    ("force_scan_forest", _in(force_scan=1, n_trees=5), _plan(EXACT, 1, n_out=5)),
    # one stream-eligible ruleset
    ("stream_64", _in(n=64), _plan(STREAM, 1, rows_stride=11)),
    ("stream_4096", _in(n=4096), _plan(STREAM, 2, rows_stride=11)),
    ("lean_4097", _in(n=4097), _plan(LEAN, 3, stage_bytes=3000, **ORDERED)),
    ("lean_4097_no_bitmap", _in(n=4097, bitmap=0), _plan(LEAN, 3, stage_bytes=3000, **dict(ORDERED, tout_bm=0))),
    ("lean_4097_no_len_sort", _in(n=4097, len_sort=0), _plan(LEAN, 3, stage_bytes=3000)),
    ("stream_rows_by_selectors", _in(n=64, max_sel=9), _plan(STREAM, 1, rows_stride=14)),
    ("mods", _in(n=4097, mods=1), _plan(LEAN, 3, stage_bytes=3000, mods=1, **ORDERED)),
    # one ruleset the stream does not take
    ("lean_4095", _in(n=4095, all_stream=0), _plan(LEAN, 2, stage_bytes=3000)),
    ("lean_4096", _in(n=4096, all_stream=0), _plan(LEAN, 2, stage_bytes=3000, **ORDERED)),
    # forests
    ("forest5_4097", _in(n=4097, n_trees=5), _plan(LEAN, 3, stage_bytes=3000, keep_rows=1, len_order=1, n_out=5)),
    ("forest1_4097", _in(n=4097, n_trees=1), _plan(LEAN, 3, stage_bytes=3000, keep_rows=1, **ORDERED)),
    ("forest5_stream", _in(n=64, n_trees=5), _plan(STREAM, 1, rows_stride=11, keep_rows=1, n_out=5)),
    # a blob over the shared limit is not staged; a lean ablation can not run without
    ("big_blob", _in(n=4097, all_stream=0, max_blob=SHARED_MAX + 16), _plan(LEAN, 3, **ORDERED)),
    ("blob_at_limit", _in(n=4097, all_stream=0, max_blob=SHARED_MAX), _plan(LEAN, 3, stage_bytes=SHARED_MAX, **ORDERED)),
    ("big_blob_mode15", _in(n=4097, all_stream=0, max_blob=SHARED_MAX + 16, mode=15),
     _plan(INVALID, 32, abl=1, **dict(ORDERED, out_k=0))),
    # three stream-eligible rulesets
    ("mt_100", _in(n=100, **THREE), _plan(STREAM, 1, rows_stride=11, **T3)),
    ("mt_10000", _in(n=10000, **THREE), _plan(TENANT, 1, stage_bytes=TENANT_MAX, **T3)),
    ("mt_small_blobs", _in(n=10000, n_sets=3), _plan(TENANT, 1, stage_bytes=3000, **T3)),
    ("mt_len_sort2", _in(n=10000, len_sort=2, **THREE), _plan(TENANT, 1, stage_bytes=TENANT_MAX, len_order=1, **T3)),
    ("mt_no_stage", _in(n=10000, no_tenant_stage=1, **THREE), _plan(FUSED, 1, **T3)),
    ("mt_not_eligible", _in(n=100, all_stream=0, **THREE), _plan(TENANT, 1, stage_bytes=TENANT_MAX, **T3)),
    # mode 41: the lean kernel where the stream would run
    ("m41_64", _in(mode=41, n=64, n_trees=5), _plan(LEAN, 32, stage_bytes=3000, keep_rows=1, n_out=5)),
    ("m41_big", _in(mode=41, n=BIG), _plan(LEAN, 32, stage_bytes=3000, **ORDERED)),
    # mode 52: the stream at any size
    ("m52_big", _in(mode=52, n=BIG, n_trees=5), _plan(STREAM, 32, rows_stride=11, keep_rows=1, n_out=5)),
    ("m52_mt", _in(mode=52, n=100, **THREE), _plan(TENANT, 1, stage_bytes=TENANT_MAX, **T3)),
    # modes 50 / 51: the stream's profiling instances, one ruleset only
    ("m50", _in(mode=50, n=BIG, n_trees=5), _plan(STREAM, 32, rows_stride=11, stream_mode=STRUCTURAL, n_out=5)),
    ("m51", _in(mode=51, n=64), _plan(STREAM, 32, rows_stride=11, stream_mode=NO_FOLD)),
    ("m50_mt", _in(mode=50, n=10000, **THREE), _plan(TENANT, 1, stage_bytes=TENANT_MAX, **T3)),
    ("m50_not_eligible", _in(mode=50, n=BIG, all_stream=0), _plan(LEAN, 32, stage_bytes=3000)),
    # mode 53: the small-batch phase clocks
    ("m53_64", _in(mode=53, n=64, n_trees=5), _plan(STREAM, 1, rows_stride=11, stream_mode=TIMING, n_out=5)),
    ("m53_big", _in(mode=53, n=BIG), _plan(LEAN, 32, stage_bytes=3000)),
    # mode 40: the default kernels, not full
    ("m40_big", _in(mode=40, n=BIG, n_trees=5), _plan(LEAN, 32, stage_bytes=3000, n_out=5)),
    ("m40_64", _in(mode=40, n=64), _plan(LEAN, 32, stage_bytes=3000)),
] + [
    # modes 15..18: the lean ablations keep the length order and its inverse, gather nothing
    ("m%d_big" % m, _in(mode=m, n=BIG), _plan(LEAN, 32, abl=m - 14, stage_bytes=3000, **dict(ORDERED, out_k=0)))
    for m in (15, 16, 17, 18)
] + [
    ("m%d_forest" % m, _in(mode=m, n=BIG, n_trees=5), _plan(LEAN, 32, abl=m - 14, stage_bytes=3000, len_order=1, n_out=5))
    for m in (15, 18)
] + [
    ("m%d_mt" % m, _in(mode=m, n=BIG, **THREE), _plan(INVALID, 1, abl=m - 14, stage_bytes=TENANT_MAX, **T3))
    for m in (15, 16, 17, 18)
]


@pytest.mark.parametrize("name,inp,want", TABLE, ids=[t[0] for t in TABLE])
def test_plan_table(name, inp, want):
    got = H.plan_eval(**inp)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_mode_known():
    for m in MODES:
        assert H.mode_known(m), m
    for m in (1, 2, 3, 10, 11, 12, 5, 19, 42, -1, 14, 39, 49, 54):
        assert not H.mode_known(m), m
    assert [m for m in range(-5, 200) if H.mode_known(m)] == list(MODES)


def _random_inputs(count):
    rng = np.random.default_rng(7)
    ns = [0, 1, 63, 64, 2048, 4095, 4096, 4097, 10000, BIG, (1 << 32) - 4096]
    for _ in range(count):
        yield _in(n=int(rng.choice(ns)), n_sets=int(rng.integers(1, 5)), all_stream=int(rng.integers(0, 2)),
                  max_rec=int(rng.integers(0, 40)), max_sel=int(rng.integers(0, 33)),
                  max_blob=int(rng.choice([256, 3000, TENANT_MAX, 20000, SHARED_MAX, SHARED_MAX + 16, 200000])),
                  n_trees=int(rng.choice([0, 0, 1, 5])), lean_feat=int(rng.integers(0, 4)),
                  mods=int(rng.integers(0, 2)), bitmap=int(rng.integers(0, 2)), force_scan=int(rng.integers(0, 4) == 0),
                  mode=int(rng.choice(MODES + (1, 12, 42))), len_sort=int(rng.integers(0, 3)),
                  no_tenant_stage=int(rng.integers(0, 2)), stream_max_n=int(rng.choice([0, 64, 4096, BIG])))


def test_kept_rows_only_where_a_kernel_keeps_them():
    """keep_rows implies the stream or the lean path, the two whose kernels honour it (a plan
    that promised rows for another kernel would let authjx_select_from_eval_device read rows
    nobody wrote); and what follows from one another in a plan does."""
    inputs = [t[1] for t in TABLE] + list(_random_inputs(4000))
    kept = 0
    for inp in inputs:
        p = H.plan_eval(**inp)
        if p["keep_rows"]:
            kept += 1
            assert p["path"] in (STREAM, LEAN), (inp, p)
            assert inp["n_sets"] == 1 and inp["n_trees"] != 0 and p["abl"] == 0, (inp, p)
        assert p["path"] <= INVALID and 1 <= p["per"] <= 32, (inp, p)
        if p["out_k"]:
            assert p["want_pos_of"] and p["path"] == LEAN and p["n_out"] == 1, (inp, p)
        if p["want_pos_of"] or p["tout_bm"]:
            assert p["len_order"], (inp, p)
        if p["len_order"]:
            assert p["path"] in (LEAN, TENANT, FUSED, INVALID) and inp["n"] >= 4096, (inp, p)
        if p["path"] == LEAN:
            assert inp["n_sets"] == 1 and p["stage_bytes"] <= SHARED_MAX, (inp, p)
        if p["path"] in (TENANT, FUSED):
            assert inp["n_sets"] > 1 and (p["stage_bytes"] != 0) == (p["path"] == TENANT), (inp, p)
            assert p["stage_bytes"] <= TENANT_MAX, (inp, p)
        if p["path"] == STREAM:
            assert inp["all_stream"] and p["rows_stride"] >= 5 + inp["max_rec"], (inp, p)
    assert kept >= 50  # (the random inputs reach it: about one in fifty keeps rows)
