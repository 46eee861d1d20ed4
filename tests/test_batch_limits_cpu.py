"""CPU: what the scenarios of tests/batch_limit_cases.py hold, on the models alone - so that a seed that drifts fails here and not
silently on the device -, the vectorised definition of the lists and the permutation against tests/minibatch_model.py and
tests/chunks_model.py element for element, the float32 Retrace model against the paper's sum in float64 within the derived bound,
and the limit scenarios through the __host__ side of the same arithmetic (the three stand-alone harnesses, their input formats
unchanged), plain and under the host's sanitizers."""
import os

import numpy as np
import pytest

import batch_limit_cases as bl
import chunks_model as cm
import minibatch_model as mm
import retrace_model as rm
import test_chunks_cpu as tc
import test_minibatch_cpu as tm
import test_retrace_cpu as tr

SEED = 5


def _same_take(got, want, keys, what):
    for key in keys:
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), (key, what)
    assert len(got["streams"]) == len(want["streams"])
    for g, w in zip(got["streams"], want["streams"]):
        assert np.array_equal(rm.bits(g), rm.bits(w)), ("streams", what)


def _minibatch_forms(total):
    return ((total // 2, 1), (max(total - 2, 0), 5), (0, 2 * total + 3), (total + 1, 4))


def _against_the_minibatch_model(a, N, L):
    model, mine = mm.Model(N, SEED), bl.Minibatches(N, SEED)
    for which in (mm.LIVE, mm.BOOT):
        for epoch in range(2):
            total = model.select(which, a["len"], a["ends"], L)
            assert mine.select(which, a["len"], a["ends"], L) == total
            assert int(mine.key[which][0]) == model.key[which]
            assert np.array_equal(np.concatenate([[0], np.cumsum(np.bincount(mine.envs[which], minlength=N))]), model.off[which])
            for permute in (False, True):
                for first, S in _minibatch_forms(total):
                    args = (a["obs_index"], a["next_index"], a["payload"], a["streams"][:2])
                    want = model.take(which, permute, a["len"], a["ends"], L, first, S, *args)
                    _same_take(mine.take(which, permute, first, S, *args), want, ("slot", "env", "valid", "obs_index", "next_index", "payload"),
                               (N, L, which, epoch, permute, first, S))


def _against_the_chunk_model(a, N, L, C, sizes=(1, 65)):
    model, mine = cm.Model(N, SEED), bl.Chunks(N, SEED)
    for epoch in range(2):
        total = model.select(a["len"], L, C)
        assert mine.select(a["len"], L, C) == total and int(mine.key[0]) == model.key
        for permute in (False, True):
            for first, S in ((0, sizes[0]), (total // 2, sizes[1]), (total + 1, 3)):
                args = (a["obs_index"], a["next_index"], a["payload"], a["streams"][:2])
                want = model.take(permute, a["len"], a["ends"], L, C, first, S, *args)
                _same_take(mine.take(permute, a["ends"], L, C, first, S, *args), want, cm.STEP_KEYS + cm.CHUNK_KEYS, (N, L, C, epoch, permute, first, S))
    if L > 1:                                                        # another (L, C) than select saw: null rows
        assert mine.take(True, a["ends"], L, C + 1 if C < L else C - 1, 0, 3)["chunk"].tolist() == [-1] * 3


# ---------------------------------------------------------------------------------------------- the vectorised definition
@pytest.mark.parametrize("N,L", tm.SHAPES)
def test_vectorised_minibatches_equal_the_scalar_model(N, L):
    _against_the_minibatch_model(mm.rollout_arrays(100 + N * 131 + L, N, L), N, L)


@pytest.mark.parametrize("N,L", tc.SHAPES)
def test_vectorised_chunks_equal_the_scalar_model(N, L):
    a = cm.rollout_arrays(100 + N * 131 + L, N, L)
    for C in tc.chunk_lengths(L):
        _against_the_chunk_model(a, N, L, C)


@pytest.mark.parametrize("N", [257, 513])
def test_vectorised_definitions_equal_the_scalar_models_on_scan(N):
    for variant in ("live", "dead"):
        a = bl.scan(N, variant)
        _against_the_minibatch_model(a, N, bl.SCAN_L)
        for C in (1, bl.SCAN_L):
            _against_the_chunk_model(a, N, bl.SCAN_L, C)


@pytest.mark.parametrize("total", sorted(bl.TOTALS))
def test_totals_are_bijections_that_reach_their_half_bits_and_walk(total):
    N, L = bl.TOTALS[total]
    a = bl.totals(total)
    mine = bl.Minibatches(N, SEED)
    assert mine.select(mm.LIVE, a["len"], a["ends"], L) == total
    assert bl.half_bits(total) == bl.TOTALS_HB[total] == mm.half_bits(total)
    walks = np.zeros(total, np.int32)
    for epoch in range(4 if total <= 17 else 1):                     # (a domain of 4 leaves [0, total) in some epochs only)
        if epoch:
            mine.select(mm.LIVE, a["len"], a["ends"], L)
        got = mine.take(mm.LIVE, True, 0, total)
        assert np.array_equal(np.sort(got["slot"]), np.sort(mine.slots[mm.LIVE])) and len(set(got["slot"].tolist())) == total and got["valid"].all()
        assert got["walks"].min() >= 1
        walks = np.maximum(walks, got["walks"])
    if total != 4 ** bl.half_bits(total):                            # not the whole domain 4^hb: some position leaves [0, total) and walks on
        assert walks.max() >= 2, total
    else:
        assert walks.max() == 1
    if total == 2 ** 20 + 1:                                         # the domain is 4 x total: three quarters of the positions walk on
        assert walks.max() >= 20 and (walks >= 2).mean() > 0.7
    if 16 < total <= 4097:                                           # ... and the scalar model agrees where it is fast enough
        assert got["slot"].tolist() == [int(mine.slots[mm.LIVE][mm.perm(int(mine.key[0][0]), total, m)]) for m in range(total)]
    print(f"total {total}: hb {bl.half_bits(total)}, walks up to {int(walks.max())}, {float((walks >= 2).mean()):.3f} of the positions walk at least twice")


def test_totals_cover_the_stated_half_bits():
    assert set(bl.TOTALS_HB.values()) == {1, 2, 3, 7, 9, 10, 11} and sorted(bl.TOTALS) == [1, 2, 3, 4, 5, 16, 17, 4097, 65537, 2 ** 20, 2 ** 20 + 1]
    assert {t.bit_length() % 2 for t in bl.TOTALS if t > 1} == {0, 1}          # both parities of the bit length


# ---------------------------------------------------------------------------------------------- what the scenarios hold
def _zero_runs(counts):
    """[(from, to)] of the maximal runs of zero counts."""
    z = np.concatenate([[0], (np.asarray(counts) == 0).astype(np.int8), [0]])
    d = np.diff(z)
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


@pytest.mark.parametrize("N", bl.SCAN_NS)
def test_scan_holds_the_zero_runs_it_claims(N):
    L = bl.SCAN_L
    for variant in bl.SCAN_VARIANTS:
        a = bl.scan(N, variant)
        for which in (mm.LIVE, mm.BOOT):
            counts = mm.selected(which, a["len"], a["ends"], L).sum(0)
            if variant == "full":
                assert which == mm.BOOT or (counts == L).all()
                continue
            assert (counts[0] > 0) == (counts[N - 1] > 0) == (variant == "live") or which == mm.BOOT
            runs = _zero_runs(counts)
            if N >= 512:
                assert any(a_ <= 128 and b_ >= 384 for a_, b_ in runs), "no run of 256 empty envs across the scan's first run boundary"
            if N >= 513:
                end = N if variant == "dead" else N - 1
                assert any(b_ >= end and b_ - a_ >= 256 for a_, b_ in runs), "no run of 256 empty envs at the end"
            if N > 256:                                              # wave 3's `before` and the carried total are both non-zero
                assert counts[:192].sum() > 0 and counts[:256].sum() > 0
                assert counts[256:].sum() > 0 or variant == "dead" or which == mm.BOOT      # ("dead" at 257 and 513: the second run adds nothing)
        chunks = np.diff(cm.offsets(a["len"], L, 1))
        assert np.array_equal(chunks, np.clip(a["len"], 0, L))          # C = 1: a chunk per live step
    assert (np.clip(bl.scan(N, "live")["len"], 0, L) != bl.scan(N, "live")["len"]).any()


@pytest.mark.parametrize("N,L", bl.DEEP)
def test_deep_holds_the_two_column_walk_extremes(N, L):
    a = bl.deep(N, L)
    assert L == 4096 and a["len"][bl.DEEP_TOP] == L and a["len"][bl.DEEP_BOTTOM] == L
    boot = (a["ends"] & 8) != 0
    assert np.nonzero(boot[:, bl.DEEP_TOP])[0].tolist() == [0] and np.nonzero(boot[:, bl.DEEP_BOTTOM])[0].tolist() == [L - 1]
    assert set(np.unique(a["ends"]).tolist()) == set(range(16))
    mine = bl.Minibatches(N, SEED)
    live, boots = mine.select(mm.LIVE, a["len"], a["ends"], L), mine.select(mm.BOOT, a["len"], a["ends"], L)
    assert live > 100000 * (N // 65) and boots > live // 3
    assert {0 * N + bl.DEEP_TOP, (L - 1) * N + bl.DEEP_BOTTOM} <= set(mine.slots[mm.BOOT].tolist())
    print(f"deep ({N}, {L}): LIVE {live}, BOOT {boots}")


@pytest.mark.parametrize("L,C", bl.CHUNKY)
def test_chunky_holds_a_late_first_step_and_a_short_last_chunk(L, C):
    G = cm.groups(L, C)
    assert (L, C, G) in ((256, 256, 1), (257, 256, 2), (4096, 256, 16), (4096, 255, 17), (4096, 1, 4096), (4095, 256, 16))
    for N in bl.CHUNKY_NS:
        a = bl.chunky(N, L, C)
        t0 = L - np.clip(a["len"], 0, L)
        assert tuple(t0[:4].tolist()) == bl.chunky_t0(L, C) and a["len"][4] == 0
        assert t0[1] % C == 0 and (t0[2] % C == C - 1 or t0[2] == L - 1) and t0[3] == L - 1
        mine = bl.Chunks(N, SEED)
        total = mine.select(a["len"], L, C)
        got = mine.take(False, a["ends"], L, C, 0, total)
        if C > 1:
            assert (got["first"] > 0).any(), "no chunk whose first live step lies behind its first step"
            assert (got["first"] == C - 1).any() or L - 1 - (G - 1) * C < C - 1
        if L % C:
            short = got["chunk"] == G - 1
            assert short.any() and (got["steps"][short] <= L % C).all() and (got["steps"][short] == L % C).any(), "no short last chunk"
            assert (got["slot"][L % C:, short] == -1).all()
        assert (got["steps"] >= 1).all() and ((got["slot"] >= 0).sum(0) == got["steps"]).all()
        assert (got["start"] & cm.START_EPISODE).any() and int((got["start"] & cm.START_CHUNK != 0).sum()) == total
    if (L, C) == (4096, 255):
        assert L % C == 16
    if (L, C) == (4096, 1):
        assert G == 4096


def test_state_index_and_start_bits_at_a_chunk_boundary_and_behind_an_episode_end():
    """t0 on a chunk's first step: START_CHUNK at l = 0 and state_index the observation there; an episode end in the last step of
    the chunk before: START_CHUNK | START_EPISODE at l = 0 of the next chunk - against the scalar model."""
    N, L, C = 5, 257, 256
    a = {k: (v.copy() if isinstance(v, np.ndarray) else [s.copy() for s in v]) for k, v in bl.chunky(N, L, C).items()}
    a["ends"][C - 1, 0] |= 1                                         # env 0 (t0 = 0): the episode ends on the last step of chunk 0
    model, mine = cm.Model(N, SEED), bl.Chunks(N, SEED)
    total = model.select(a["len"], L, C)
    assert mine.select(a["len"], L, C) == total
    want = model.take(False, a["len"], a["ends"], L, C, 0, total, a["obs_index"], a["next_index"])
    got = mine.take(False, a["ends"], L, C, 0, total, a["obs_index"], a["next_index"])
    _same_take(got, dict(want, streams=[]), cm.STEP_KEYS[:4] + cm.STEP_KEYS[5:] + cm.CHUNK_KEYS, "boundary")
    assert got["env"][0, 1] == 0 and got["chunk"][1] == 1 and got["start"][0, 1] == cm.START_CHUNK | cm.START_EPISODE
    assert got["state_index"][1] == a["obs_index"][C, 0]


def test_far_positions_wrap_onto_real_samples():
    N, L = bl.MID
    a = bl.mid()
    mine = bl.Minibatches(N, SEED)
    total = mine.select(mm.LIVE, a["len"], a["ends"], L)
    for S in bl.FAR_SIZES:
        first = bl.INT32_MAX - S
        got = mine.take(mm.LIVE, True, first, S, a["obs_index"])
        assert not got["valid"].any() and (got["slot"] >= 0).all() and first + S == bl.INT32_MAX and first >= total
        want = [mm.perm(int(mine.key[0][0]), total, (first + i) % total) for i in range(S)]
        assert got["slot"].tolist() == mine.slots[mm.LIVE][want].tolist()


# ---------------------------------------------------------------------------------------------- Retrace
def test_retrace_edges_are_the_stated_shapes():
    assert len(bl.EDGES) == 33 and (4097, 9) in bl.EDGES and (65, 256) in bl.EDGES
    assert {L % 8 for _, L in bl.EDGES} >= {7, 0, 1} and -(-4097 // 64) == 65 and 4097 % 64 == 1
    live = sum(bool(np.isnan(rm.retrace(**bl.edge(B, L))[0]).any()) for B, L in bl.EDGES)
    assert live >= 10                                                # NaN at steps with a row in every other shape


def test_retrace_special_holds_every_kind_in_both_outputs():
    k = bl.special()
    B, L = bl.SPECIAL_SHAPE
    has = rm.has_row(k["length"], k["steps"])
    inside = np.arange(L)[None, :] < np.clip(k["length"], 0, L)[:, None]
    for name in ("reward", "discount", "q", "v", "c"):
        read = inside if name == "v" else has
        assert np.isnan(k[name][~read]).all(), name                  # NaN wherever the rule says the value is not read
        got = set(rm.bits(k[name][read]).tolist())
        assert set(rm.bits(bl.SPECIAL_VALUES[:-1]).tolist()) <= got and np.isnan(k[name][read]).any(), name
    assert set(rm.bits(bl.SPECIAL_VALUES[[1, 4, 6, 10]]).tolist()) <= set(rm.bits(k["boot"]).tolist())
    for boot in (True, False):
        target, td, valid = rm.retrace(**(k if boot else dict(k, boot=None)))
        for name, x in (("target", target), ("td", td)):
            found = bl.kinds(x)
            assert all(found.values()), (name, boot, found)
            assert not rm.bits(x)[~has].any()                        # +0.0 where there is no row, under NaN in everything around it
            print(f"special, boot {boot}, {name}: {found}")


@pytest.mark.parametrize("B,L", bl.DEFINITION_SHAPES)
def test_float32_model_lies_within_the_derived_bound_of_the_papers_sum(B, L):
    for boot in (True, False):
        k, d = bl.plain(B, L), bl.definition(B, L, boot)
        target, td, valid = rm.retrace(**(k if boot else dict(k, boot=None)))
        assert np.array_equal(valid != 0, d["has"]) and d["has"].sum() > B
        assert not d["left_out"].any(), "a step is left out of the comparison: choose other inputs"
        assert np.isfinite(target).all() and np.isfinite(d["target"]).all() and d["longest"] >= min(L, 9)
        worst = bl.worst_ratio(target, td, d)
        print(f"({B}, {L}), boot {boot}: {int(d['has'].sum())} steps, chains up to {d['longest']}, worst error / bound: target {worst[0]:.3f}, td {worst[1]:.3f}")
        assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
        assert worst[0] > 0.01, "the bound is vacuous"


def test_the_bound_sees_a_contracted_or_misread_fold():
    """The check has teeth on the model: reading discount one step late, or dropping the product with c, leaves the bound by
    orders of magnitude."""
    B, L = bl.DEFINITION_SHAPES[0]
    k, d = bl.plain(B, L), bl.definition(B, L)
    wrong = rm.retrace(**dict(k, c=np.ones_like(k["c"])))
    assert bl.worst_ratio(wrong[0], wrong[1], d)[0] > 1000


# ---------------------------------------------------------------------------------------------- the harnesses
def _mb_harness(binary, tmp_path, a, N, L, takes):
    """counts of both lists, and takes = [(which, permute, first, S)] against the vectorised definition."""
    mine = bl.Minibatches(N, SEED)
    for which in (mm.LIVE, mm.BOOT):
        total = mine.select(which, a["len"], a["ends"], L)
        counts = np.bincount(mine.envs[which], minlength=N)
        got = [r[0] for r in tm._run(binary, tmp_path, [1, which, N, L, *a["len"].tolist(), *a["ends"].reshape(-1).tolist()])]
        assert got == counts.tolist() and sum(got) == total
        off = np.concatenate([[0], np.cumsum(counts)])
        for w, permute, first, S in takes:
            if w != which:
                continue
            first = first if first >= 0 else total + first
            got = np.array(tm._run(binary, tmp_path, [2, which, permute, N, L, first, S, *tm._u64(int(mine.key[which][0])), *off.tolist(),
                                                      *a["len"].tolist(), *a["ends"].reshape(-1).tolist()]), np.int64)
            want = mine.take(which, bool(permute), first, S)
            assert np.array_equal(got[:, 0], want["slot"]) and np.array_equal(got[:, 1], want["env"]) and np.array_equal(got[:, 2], want["valid"]), (which, permute, first, S)


def _check_mb_harness(binary, tmp_path):
    N = 513
    for variant in ("live", "dead"):
        _mb_harness(binary, tmp_path, bl.scan(N, variant), N, bl.SCAN_L, [(w, p, 0, 3000) for w in (0, 1) for p in (0, 1)])
    N, L = bl.DEEP[0]
    _mb_harness(binary, tmp_path, bl.deep(N, L), N, L, [(0, 1, 0, 600), (0, 0, -300, 600), (1, 1, 0, 600), (1, 0, -300, 600)])


def test_minibatch_harness_on_scan_and_deep(tmp_path_factory, tmp_path):
    if not os.path.exists(tm.HIPCC):
        pytest.skip("hipcc not found")
    _check_mb_harness(tm._compile(str(tmp_path_factory.mktemp("harness") / "minibatch_harness")), tmp_path)


def test_minibatch_harness_on_scan_and_deep_under_sanitizers(tmp_path_factory, tmp_path):
    if not os.path.exists(tm.HIPCC):
        pytest.skip("hipcc not found")
    _check_mb_harness(tm._compile(str(tmp_path_factory.mktemp("harness_san") / "minibatch_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                  "-Xarch_host", "-fno-sanitize-recover=undefined"), tmp_path)


def _chunk_harness(binary, tmp_path, a, N, L, C, takes):
    mine = bl.Chunks(N, SEED)
    total = mine.select(a["len"], L, C)
    counts = np.bincount(mine.n, minlength=N)
    got = [r[0] for r in tc._run(binary, tmp_path, [1, N, L, C, *a["len"].tolist()])]
    assert got == counts.tolist() and sum(got) == total
    off = np.concatenate([[0], np.cumsum(counts)])
    for permute, first, S in takes:
        first = first if first >= 0 else total + first
        got = np.array(tc._run(binary, tmp_path, [2, permute, N, L, C, first, S, L, C, *tc._u64(int(mine.key[0])), *off.tolist(), *a["len"].tolist(),
                                                  *a["ends"].reshape(-1).tolist()]), np.int64).reshape(S, 5 + 4 * C)
        want = mine.take(bool(permute), a["ends"], L, C, first, S)
        for k, key in enumerate(("chunk", "first", "steps", "valid")):
            assert np.array_equal(got[:, k], want[key]), (key, N, L, C, permute, first, S)
        assert np.array_equal(got[:, 4], want["env"][0])
        for k, key in enumerate(("slot", "ends", "start", "mask")):
            assert np.array_equal(got[:, 5 + k::4].T, want[key]), (key, N, L, C, permute, first, S)


def _check_chunk_harness(binary, tmp_path):
    for variant in ("live", "dead"):
        for C in (1, bl.SCAN_L):
            _chunk_harness(binary, tmp_path, bl.scan(513, variant), 513, bl.SCAN_L, C, [(0, 0, 2500), (1, 0, 2500)])
    for N in bl.CHUNKY_NS:
        _chunk_harness(binary, tmp_path, bl.chunky(N, 4096, 255), N, 4096, 255, [(0, 0, 40), (1, 0, 65), (0, -5, 9)])


def test_chunks_harness_on_scan_and_chunky(tmp_path_factory, tmp_path):
    if not os.path.exists(tc.HIPCC):
        pytest.skip("hipcc not found")
    _check_chunk_harness(tc._compile(str(tmp_path_factory.mktemp("harness") / "chunks_harness")), tmp_path)


def test_chunks_harness_on_scan_and_chunky_under_sanitizers(tmp_path_factory, tmp_path):
    if not os.path.exists(tc.HIPCC):
        pytest.skip("hipcc not found")
    _check_chunk_harness(tc._compile(str(tmp_path_factory.mktemp("harness_san") / "chunks_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                     "-Xarch_host", "-fno-sanitize-recover=undefined"), tmp_path)


def _check_retrace_harness(binary, tmp_path):
    k = bl.special()
    for time_major in (False, True):
        for boot in (True, False):
            want = rm.retrace(**(k if boot else dict(k, boot=None)))
            got = tr._harness(binary, tmp_path, k, time_major, boot)
            assert rm.same(got[0], want[0]) and rm.same(got[1], want[1]) and np.array_equal(got[2], want[2]), (time_major, boot)
            assert all(bl.kinds(got[0]).values()) and all(bl.kinds(got[1]).values())


def test_retrace_harness_on_special(tmp_path_factory, tmp_path):
    if not os.path.exists(tr.HIPCC):
        pytest.skip("hipcc not found")
    _check_retrace_harness(tr._compile(str(tmp_path_factory.mktemp("harness") / "retrace_harness")), tmp_path)


def test_retrace_harness_on_special_under_sanitizers(tmp_path_factory, tmp_path):
    if not os.path.exists(tr.HIPCC):
        pytest.skip("hipcc not found")
    _check_retrace_harness(tr._compile(str(tmp_path_factory.mktemp("harness_san") / "retrace_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                       "-Xarch_host", "-fno-sanitize-recover=undefined"), tmp_path)
