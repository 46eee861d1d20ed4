"""The scenarios of tests/limit_cases.py, checked on the models alone - before any GPU run: that each one holds what the GPU
modules (tests/test_gpu_sampler_limits.py, tests/test_gpu_steplog_limits.py, tests/test_gpu_rollout_launch.py) count on it for, so
that a seed that drifts fails here and not silently on the device; that rollout_model.gae_vec is gae bit for bit; that the
float64 definitions and their bounds hold on the float32 models; and the host side of the step log's fold
(tests/steplog_harness.cpp), plain and under the host's sanitizers, on the special-float rows.  No GPU involved."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import limit_cases as lc
import priority_model as pm
import replay_model as rm
import rollout_model as ro
import steplog_model as sm
from steplog_model import bits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------------------------------------- span, span17
@pytest.fixture(scope="module")
def span():
    return lc.span_model("span")[1]


def test_span_is_the_scenario_the_issue_states(span):
    """The figures the scenario was chosen by: counts, the saturated age byte, inspect's ahead = 255, the accepted set and the
    prioritized draw at (64, 64)."""
    assert lc.SPAN_LIMIT == 64 and max(max(c) for c in lc.SPAN_CONFIGS) == lc.SPAN_LIMIT
    assert span.count.tolist() == [356, 351, 371, 363, 363] and int(span.age.max()) == 255
    ahead = [rm.inspect(span, 0, k)[1] for k in range(-1, int(span.count[0]) + 1)]
    assert sum(a == 255 for a in ahead) == 62 and max(ahead) == 255
    assert len(rm.accepted_set(span, 64, 64)) == 834
    _, _, ok, _, _, acc = pm.draw(span, pm.Table(span), 64, 64, lc.SAMPLER_SEED, 0, lc.SPAN_B)
    assert ok.all() and acc == 834


@pytest.mark.parametrize("name", sorted(lc.SPAN))
@pytest.mark.parametrize("back, forward", lc.SPAN_CONFIGS)
def test_span_reaches_across_chunks(name, back, forward):
    """Each config's accepted set is non-empty and smaller than the candidate set (rejections happen), holds samples whose
    k - back lies in an earlier chunk of 64 positions than k (back > 0) and samples whose k + forward lies in a later one
    (forward > 0); on `span` an accepted k has a saturated age."""
    model = lc.span_model(name)[1]
    r = lc.span_reach(model, back, forward)
    assert 0 < r["accepted"] < r["candidates"], r
    assert (r["behind"] > 0) == (back > 0) and (r["ahead"] > 0) == (forward > 0), r
    if name == "span":
        assert r["saturated"] >= 1, r
    else:
        assert model.N % 16 == 1                             # the last k_priority_weights group holds one env


def test_span_draw_points_and_the_set_draw(span):
    """The two earlier draws happen while every count is below T, with a non-empty accepted set for every config at the later
    one; and B = SPAN_SET_B equally weighted draws reach every member of each accepted set."""
    N, fs, T, steps, at = lc.SPAN["span"]
    assert at[-1] == steps - 1
    for i, upto in enumerate(at[:-1]):
        model = lc.span_model("span", upto + 1)[1]
        assert int(model.count.max()) < T
        acc = [len(rm.accepted_set(model, b, f)) for b, f in lc.SPAN_CONFIGS]
        assert all(a > 0 for a in acc) or i == 0, acc
    for back, forward in lc.SPAN_CONFIGS:
        env, idx, ok, _, _, acc = pm.draw(span, pm.Table(span), back, forward, 5, 0, lc.SPAN_SET_B)
        assert ok.all() and sorted(set(zip(env.tolist(), idx.tolist()))) == rm.accepted_set(span, back, forward) and acc > 800


def test_span_tables_hold_many_weights(span):
    table, rows, prio = lc.span_table(span, 2)
    assert len(rows) == 5 * 320 and len(set(table.weight.reshape(-1).tolist())) > 1000 and table.wmax > pm.ONE


# ---------------------------------------------------------------------------------------------- deepfold
@pytest.fixture(scope="module")
def deepfold():
    return lc.Deep("deepfold")


def test_deepfold_folds_64_rows_and_stops_for_every_reason(deepfold):
    d = deepfold
    lm = d.logs[4]
    samples = d.samples()
    res = [lc.stop_reason(d.hm, lm, n, k, lc.NSTEP_LIMIT) for n, k in samples]
    assert (64, "nstep") in res
    for why in ("history", "age0", "unrecorded", "flag"):
        assert any(1 <= m <= 63 and w == why for m, w in res), why
    assert any(m == 0 and w == why for m, w in res for why in ("invalid",))
    # the wave that leaves the loop by __any: 64 consecutive samples with a 64-row fold and a 0-row one
    groups = [g for g in range(0, len(samples), 64) if (64, "nstep") in res[g:g + 64] and any(m == 0 for m, _ in res[g:g + 64])]
    assert groups
    # stop_reason is the model's walk
    for (n, k), (m, _) in zip(samples, res):
        assert lm.gather(n, k, lc.NSTEP_LIMIT, 0.99)[0] == m
    assert {1, 63, 64} <= {m for m, _ in res} and int(d.hm.count.max()) > d.T           # the ring wrapped


def test_deepfold_logs_share_rows_and_differ_in_width(deepfold):
    d = deepfold
    a, b = d.logs[4], d.logs[64]
    assert np.array_equal(a.stamp, b.stamp) and np.array_equal(bits(a.reward), bits(b.reward)) and np.array_equal(a.flags, b.flags)
    assert np.array_equal(a.payload, b.payload[:, :, :4]) and b.payload.shape[2] == lc.PAYLOAD_LIMIT == 64
    assert np.array_equal(a.stamp, d.special.stamp) and np.array_equal(a.flags, d.special.flags)
    assert all(bits(d.rows[(n, int(a.stamp[t, n]))][0]) == bits(a.reward[t, n]) for t, n in zip(*np.nonzero(a.stamp >= 0)))
    rolls = [len(ro.rollout(a, n, lc.WIDTH_LS[1])) for n in range(d.N)]          # the rollout gathers of the payload test:
    assert 64 < min(rolls) and max(rolls) < lc.WIDTH_LS[1] and lc.WIDTH_LS[0] < 64      # every env full at one L, padded at the other


@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.5])
def test_nstep_definition_holds_on_the_model(deepfold, gamma):
    """The float64 definition against the float32 model within the derived bounds, and the share of samples the check leaves
    out (a non-zero term below 2^-100): under 5 % - none, in fact."""
    d = deepfold
    lm = d.logs[4]
    checked = left_out = 0
    worst = 0.0
    for n, k in d.samples():
        m, _, G, disc, last, _ = lm.gather(n, k, lc.NSTEP_LIMIT, gamma)
        if not m:
            continue
        ret, gm, terminated, S, smallest = lc.nstep_definition(d.rows, n, k, m, gamma)
        if smallest < lc.TINY:
            left_out += 1
            continue
        rb, db = lc.nstep_bounds(m, S, gm)
        assert abs(float(G) - ret) <= rb and terminated == bool(last & sm.TERMINATED)
        assert float(disc) == 0.0 if terminated else abs(float(disc) - gm) <= db
        worst = max(worst, abs(float(G) - ret) / rb if rb else 0.0)
        checked += 1
    assert checked > 500 and left_out == 0 and 0 < worst < 1


def test_special_log_holds_every_special_result(deepfold):
    """On the model, at nstep = 64 and gamma = 2^-3: a subnormal ret, an infinite one, an inf - inf = NaN ret (no NaN among its
    rewards), a subnormal discount and one that underflowed to 0; at gamma = 1 a ret that OVERFLOWED to inf (finite rewards
    only); and every value of the special set was recorded."""
    d = deepfold
    lm = d.special
    seen = dict(sub=0, inf=0, overflow=0, nan=0, dsub=0, dzero=0)
    with np.errstate(all="ignore"):
        for n, k in d.samples():
            m, _, G, disc, last, _ = lm.gather(n, k, lc.NSTEP_LIMIT, lc.SPECIAL_GAMMA)
            if not m:
                continue
            rw = np.array([lm.reward[(k + i) % d.T, n] for i in range(1, m + 1)])
            seen["sub"] += G != 0 and abs(G) < 2.0 ** -126
            seen["inf"] += bool(np.isinf(G))
            seen["nan"] += bool(np.isnan(G)) and not np.isnan(rw).any() and np.inf in rw[:40] and -np.inf in rw[:40]
            seen["dsub"] += disc != 0 and disc < 2.0 ** -126
            seen["dzero"] += disc == 0 and not last & sm.TERMINATED
            G1 = lm.gather(n, k, lc.NSTEP_LIMIT, 1.0)[2]
            seen["overflow"] += bool(np.isinf(G1)) and bool(np.isfinite(rw).all())
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen
    recorded = lm.reward[lm.stamp >= 0]
    for v in lc.SPECIAL:
        assert (np.isnan(recorded).any() if np.isnan(v) else (bits(recorded) == bits(v)).any()), v
    assert lc.SPECIAL_GAMMA == 2.0 ** -3 and float(np.float32(0.5) ** 64) >= 2.0 ** -126          # why gamma = 0.5 does not reach it


# ---------------------------------------------------------------------------------------------- the host side of the fold
def _compile(out, *extra):
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", *extra, "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "active-gym_amd", "csrc"), os.path.join(REPO, "tests", "steplog_harness.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness") / "steplog_harness"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """The same stand-alone program under the host's address and undefined-behaviour sanitizers."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    return _compile(str(tmp_path_factory.mktemp("harness_san") / "steplog_harness_san"), "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined")


def _check_harness(binary, tmp_path, d):
    """agx_steplog_fold.h's host side on the special rows (gamma = 2^-3 and 1) and on the ordinary ones (0.99), nstep = 64, every sample:
    NaN where the model's value is NaN, the model's bit pattern everywhere else."""
    samples = d.samples()
    for lm, gamma in ((d.special, lc.SPECIAL_GAMMAS[0]), (d.special, lc.SPECIAL_GAMMAS[1]), (d.logs[4], 0.99)):
        h = d.hm
        tok = [h.T, h.N, lc.NSTEP_LIMIT, int(bits(gamma))] + h.count.tolist() + h.age.ravel().tolist() + lm.stamp.ravel().tolist()
        tok += lm.reward.view(np.uint32).ravel().tolist() + lm.flags.ravel().tolist()
        for n, k in samples:
            tok += [n, k]
        path = tmp_path / "case.txt"
        path.write_text("\n".join(str(int(t)) for t in tok))
        r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(samples)
        nans = 0
        with np.errstate(all="ignore"):
            for (n, k), line in zip(samples, lines):
                m, nxt, G, disc, last, _ = lm.gather(n, k, lc.NSTEP_LIMIT, gamma)
                if m == 0:
                    assert line == "0 -1 - - -", (n, k)
                    continue
                f = line.split()
                assert [int(f[0]), int(f[1]), int(f[2])] == [m, nxt, last], (n, k)
                got = np.array([int(f[3]), int(f[4])], np.uint32).view(np.float32)
                for g, w in zip(got, (G, disc)):
                    if np.isnan(w):
                        assert np.isnan(g), (n, k)
                        nans += 1
                    else:
                        assert bits(g) == bits(w), (n, k, g, w)
        assert (nans > 0) == (lm is d.special)


def test_host_side_of_the_fold_on_special_floats(harness, tmp_path, deepfold):
    _check_harness(harness, tmp_path, deepfold)


def test_host_side_of_the_fold_on_special_floats_under_sanitizers(harness_san, tmp_path, deepfold):
    _check_harness(harness_san, tmp_path, deepfold)


# ---------------------------------------------------------------------------------------------- deeproll, wide
def test_deeproll_is_longer_than_1024_and_below_the_limit():
    d = lc.Deep("deeproll")
    lens = [len(ro.rollout(d.logs[4], n, ro.ROLLOUT_LIMIT)) for n in range(d.N)]
    print(lens)
    assert max(lens) > 1024 and max(lens) < ro.ROLLOUT_LIMIT == 4096 and min(lens) < 64 and any(64 < m < 1000 for m in lens)
    assert ro.features(d.logs[4], 1024) >= ro.FEATURES - {"empty"}
    for N in (1, 4):                                           # the first N envs of the same script are the same envs
        sub = lc.Deep("deeproll", N=N)
        assert [len(ro.rollout(sub.logs[4], n, ro.ROLLOUT_LIMIT)) for n in range(N)] == lens[:N]
    assert lens[0] > 64                                        # N = 1: one wave in one block, more than one pass


def test_wide_holds_every_kind_of_rollout_across_blocks():
    """N = 257: 65 blocks of k_rollout_gather, the last with one wave; full, partial and empty envs, every ends bit."""
    d = lc.Deep("wide")
    assert d.N == 257 and ro.features(d.logs[4], 8) == ro.FEATURES
    lens = np.array([len(ro.rollout(d.logs[4], n, 8)) for n in range(d.N)])
    assert len(set(lens[252:].tolist())) >= 2                  # the envs of the last two blocks differ


# ---------------------------------------------------------------------------------------------- GAE
def test_gae_vec_is_gae_bit_for_bit():
    """On the existing cases, every L, every (gamma, lambda), with and without a boot buffer, and with wild lengths."""
    for name, case in ro.CASES.items():
        _, hm, lm = ro.case_models(name)
        for L in case[5]:
            out = ro.gather(lm, L)
            value, boot = ro.gae_inputs(out, L)
            wild = np.array([-3, L + 7, 0, L, 1], np.int32)
            for gamma, lam in ro.GAMMA_LAMBDA:
                for length, ends, b in ((out["len"], out["ends"], boot), (out["len"], out["ends"] & 7, None), (wild, out["ends"], boot)):
                    want = ro.gae(length, out["reward"], ends, value, b, gamma, lam)
                    got = ro.gae_vec(length, out["reward"], ends, value, b, gamma, lam)
                    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (name, L, gamma, lam)


def test_gae_vec_is_gae_on_synthetic_and_special_inputs():
    """... and on the synthetic inputs of tests/test_gpu_rollout_launch.py at small shapes: NaN in dead slots and unused boot
    values, and the special values (NaN-ness equal, every other element bit-equal)."""
    for N, L, special in ((7, 17, False), (3, 33, False), (7, 33, True), (5, 16, True)):
        length, reward, ends, value, boot, live = lc.gae_case(N, L, N * 100 + L, special)
        for gamma, lam in ro.GAMMA_LAMBDA:
            for b, e in ((boot, ends), (None, ends & 7)):
                want = ro.gae(length, reward, e, value, b, gamma, lam)
                got = ro.gae_vec(length, reward, e, value, b, gamma, lam)
                for g, w in zip(got, want):
                    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(bits(g)[~np.isnan(w)], bits(w)[~np.isnan(w)])
                    assert not g[~live].any()
                    assert special or np.isfinite(g).all()


def test_gae_case_holds_what_it_is_there_for():
    length, reward, ends, value, boot, live = lc.gae_case(65, 33, 1, special=True)
    assert {-3, 40, 0, 33, 1} <= set(length.tolist()) and length[-1] == 33
    assert set(ends.reshape(-1).tolist()) == {0, 1, 8, 10, 12}
    assert np.isnan(boot[(ends & ro.BOOT) == 0]).all() and np.isnan(reward[~live]).all() and np.isnan(value[~live]).all()
    for arr in (reward[live], value[live], boot[live & ((ends & ro.BOOT) != 0)]):
        for v in lc.SPECIAL:
            assert (np.isnan(arr).any() if np.isnan(v) else (bits(arr) == bits(v)).any()), v
    adv, ret = ro.gae_vec(length, reward, ends, value, boot, 0.99, 0.95)
    sub = (adv != 0) & (np.abs(adv) < 2.0 ** -126)
    assert np.isnan(adv).any() and np.isinf(adv).any() and sub.any()


@pytest.mark.parametrize("gamma, lam", ro.GAMMA_LAMBDA)
def test_gae_definition_holds_on_the_model(gamma, lam):
    """The float64 definition against the float32 model within the derived bound over the live slots, ret = fl(adv + value)
    exactly, and the share the check leaves out (a non-zero term below 2^-100): none."""
    worst, checked = 0.0, 0
    for N, L in ((65, 48), (7, 4096 // 16)):
        length, reward, ends, value, boot, live = lc.gae_case(N, L, 3)
        adv, ret = ro.gae_vec(length, reward, ends, value, boot, gamma, lam)
        want, S, chain, smallest, dlive = lc.gae_definition(length, reward, ends, value, boot, gamma, lam)
        assert np.array_equal(dlive, live) and not (smallest[live] < lc.TINY).any()
        err, bound = np.abs(adv.astype(np.float64) - want)[live], lc.gae_bound(S, chain)[live]
        assert (err <= bound).all() and (bound > 0).all()
        assert np.array_equal(bits(ret[live]), bits((adv[live] + value[live]).astype(np.float32)))
        worst, checked = max(worst, float((err / bound).max())), checked + int(live.sum())
        assert int(chain[live].max()) >= 10
    assert checked > 1000 and 0 < worst < 1
