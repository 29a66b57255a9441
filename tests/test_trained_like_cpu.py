"""CPU: the instrument of test_gpu_net_trained_like.py, proven before it is pointed at a kernel (tests/trained_like.py).

The construction is what it claims (activations of rms about 1, half of them cut by the ReLUs, a pi with a top move, a V that spreads),
the factors F that bound a route's error are derived here from the fp64 reference and its fp32 proxy alone, and every defect the GPU
test must have teeth against moves the outputs by at least ten times what it allows."""
import numpy as np
import pytest
import torch

import trained_like as tl

_cache = {}


def _case(name, seed=None):
    """the net of CASES[name] (at its own seed, the GPU test's net, or at `seed`) with T, E and P (both head variants of the latter
    two), computed once"""
    _, n, blocks, dim, rows, scale, seed0 = next(c for c in tl.CASES if c[0] == name)
    seed = seed0 if seed is None else seed
    key = (name, seed)
    if key not in _cache:
        s = tl.feature_rows(n, rows, tl.FEATURE_SEED)
        net = tl.build(n, blocks, dim, seed, s, scale)
        W = tl.weights(net)
        c = dict(n=n, blocks=blocks, dim=dim, rows=rows, scale=scale, seed=seed, s=s, net=net, W=W, T=tl.forward(W, s, "truth"))
        for heads in ("native", "eager"):
            c["E", heads] = tl.forward(W, s, "emu", heads)
            c["P", heads] = tl.forward(W, s, "proxy", heads)
        _cache[key] = c
    return _cache[key]


NAMES = [c[0] for c in tl.CASES]


# ------------------------------------------------------------------------------------------------ the feature rows

@pytest.mark.parametrize("n,rows", [(9, 16), (19, 8)])
def test_feature_rows_are_shaped_as_a_game_leaves_them(n, rows):
    s = tl.feature_rows(n, rows, tl.FEATURE_SEED)
    assert s.dtype == torch.float16 and tuple(s.shape) == (rows, 18, n, n)
    assert torch.equal(s, tl.feature_rows(n, rows, tl.FEATURE_SEED)) and not torch.equal(s, tl.feature_rows(n, rows, tl.FEATURE_SEED + 1))
    a = s.numpy().astype(np.int64)
    assert set(np.unique(a)) == {0, 1}
    for t in range(8):
        assert (a[:, 2 * t] * a[:, 2 * t + 1]).sum() == 0                 # the two colours are disjoint
        if t:
            for col in (0, 1):                                            # the older plane lies inside the newer one of its colour
                assert (a[:, 2 * t + col] <= a[:, 2 * t - 2 + col]).all()
            stones = lambda u: a[:, 2 * u].sum(axis=(1, 2)) + a[:, 2 * u + 1].sum(axis=(1, 2))
            assert (stones(t) == stones(t - 1) - 1).all()                     # one ply earlier: one stone less
    assert (a[:, 0].sum(axis=(1, 2)) > n).all() and (a[:, 1].sum(axis=(1, 2)) > n).all()
    for r in range(rows):                                                 # one colour plane is all ones, the other all zeros; they alternate
        assert a[r, 16 + (r & 1)].min() == 1 and a[r, 17 - (r & 1)].max() == 0


# ------------------------------------------------------------------------------------------------ the construction

@pytest.mark.parametrize("name", NAMES)
def test_the_net_is_what_build_claims(name):
    c = _case(name)
    T, scale = c["T"], c["scale"]
    for p in c["net"].parameters():
        assert p.dtype == torch.float16 and bool(torch.isfinite(p).all())
    rms = [float(np.sqrt((a ** 2).mean())) for a in T["acts"]]
    zeros = [float((a == 0).mean()) for a in T["acts"]]
    top1 = T["pi"].max(axis=1)
    print("%s: trunk rms %s, max %.3g, zeros %s; top-1 pi %s; V %s" % (name, np.round(rms, 2), max(a.max() for a in T["acts"]),
          np.round(zeros, 2), np.round(np.sort(top1), 2), np.round(np.sort(T["V"]), 2)))
    assert len(T["acts"]) == 1 + 2 * c["blocks"]
    assert all(0.5 * scale <= r <= 3 * scale for r in rms)
    assert max(a.max() for a in T["acts"]) < 100 * scale
    share = float(np.mean([(a == 0).mean() for a in T["acts"]]))
    assert 0.2 <= share <= 0.8 and all(0.1 <= z <= 0.9 for z in zeros)
    assert np.median(top1) >= 0.3
    assert T["V"].std() >= 0.4 and np.abs(T["V"]).max() <= 0.999
    assert np.allclose(T["pi"].sum(axis=1), 1, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_the_same_seed_gives_the_same_bits(name):
    c = _case(name)
    again = tl.build(c["n"], c["blocks"], c["dim"], c["seed"], c["s"], c["scale"])
    a, b = c["net"].state_dict(), again.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    other = tl.build(c["n"], c["blocks"], c["dim"], c["seed"] + 1, c["s"], c["scale"]).state_dict()
    assert not torch.equal(a["resnet.0.upper.0.weight"], other["resnet.0.upper.0.weight"])
    T2 = tl.forward(tl.weights(again), c["s"], "truth")
    assert all(np.array_equal(T2[k], c["T"][k]) for k in ("logits", "pi", "pre", "V")) and np.array_equal(T2["acts"][-1], c["T"]["acts"][-1])


@pytest.mark.parametrize("name", NAMES)
def test_enough_rows_have_a_move_a_search_can_rely_on(name):
    """at least half the rows have a best move further ahead of the second than 8 x max |E - T| of the logits (the GPU test checks
    the argmax of exactly these rows); E and P themselves agree with T there, for the top-5 sets as well"""
    c = _case(name)
    T = c["T"]
    for heads in ("native", "eager"):
        E, P = c["E", heads], c["P", heads]
        for top in (1, 5):
            ok, want = tl.decided_rows(T, E, top)
            print("%s, %s heads: top-%d decided in %d of %d rows" % (name, heads, top, len(ok), c["rows"]))
            if top == 1:
                assert 2 * len(ok) >= c["rows"]
            for out in (E, P):
                assert np.array_equal(tl.top_sets(out["pi"], top)[ok], want[ok])


# ------------------------------------------------------------------------------------------------ the factors

def _ratios(c):
    """every ratio a factor is derived from, for one net: name -> d(P, T) / d(E, T) (or the same of the maxima)"""
    T = c["T"]
    En, Pn = c["E", "native"], c["P", "native"]
    out = {}
    blocks_and_final = range(2, len(T["acts"]), 2)       # the activation after every block; the last one is the final one
    out["trunk"] = max(tl.d(Pn["acts"][i], T["acts"][i]) / tl.d(En["acts"][i], T["acts"][i]) for i in blocks_and_final)
    out["trunk_emu"] = tl.d(Pn["acts"][-1], En["acts"][-1]) / tl.d(En["acts"][-1], T["acts"][-1])
    for heads in ("native", "eager"):
        E, P = c["E", heads], c["P", heads]
        for q in ("logits", "pi", "V"):
            out["%s/%s/rms" % (q, heads)] = tl.d(P[q], T[q]) / tl.d(E[q], T[q])
            out["%s/%s/max" % (q, heads)] = tl.dmax(P[q], T[q]) / tl.dmax(E[q], T[q])
    return out


def test_factors_are_derived_from_the_reference():
    """F(quantity) = 1.5 x the largest d(P, T) / d(E, T) over 8 seeds of every case: printed here, written into trained_like.py"""
    seen = {}
    for name in NAMES:
        seed0 = _case(name)["seed"]
        for seed in range(seed0, seed0 + tl.FACTOR_SEEDS):
            c = _case(name, seed)
            r = _ratios(c)
            E = c["E", "native"]
            print("%-12s seed %d: d(E,T) trunk %.3g logits %.3g pi %.3g V %.3g;  %s" % (
                name, seed, tl.d(E["acts"][-1], c["T"]["acts"][-1]), tl.d(E["logits"], c["T"]["logits"]), tl.d(E["pi"], c["T"]["pi"]),
                tl.d(E["V"], c["T"]["V"]), "  ".join("%s %.2f" % kv for kv in sorted(r.items()))))
            for k, v in r.items():
                seen.setdefault(k, []).append(v)
            if seed != seed0:
                del _cache[name, seed]
    print("%-18s %8s %8s %8s   F in trained_like.py" % ("quantity", "smallest", "largest", "1.5 x"))
    for k in sorted(seen):
        print("%-18s %8.3f %8.3f %8.3f   %s" % (k, min(seen[k]), max(seen[k]), 1.5 * max(seen[k]), tl.F.get(k)))
    assert sorted(seen) == sorted(tl.F) == sorted(tl.RATIOS_SEEN)
    for k in seen:
        lo, hi = tl.RATIOS_SEEN[k]
        assert 1.5 * hi - 1e-9 <= tl.F[k] <= 1.5 * hi + 0.01, k          # F is 1.5 x the largest recorded ratio, rounded up
        # The proxy's sums are this machine's (another CPU sums in another order, and V has 8 or 16 elements), so the recorded ratios
        # are not asserted to the digit: the proxy, a correct implementation, is within every bound the kernels are held to, and
        # no bound is more than 1.5 x looser than this machine's own derivation would make it.
        assert max(seen[k]) <= tl.F[k], k
        assert 1.5 * max(seen[k]) >= tl.F[k] / 1.5, k


# ------------------------------------------------------------------------------------------------ teeth

@pytest.mark.parametrize("kind", tl.MUTATIONS)
@pytest.mark.parametrize("name", NAMES)
def test_every_defect_moves_the_outputs_ten_times_beyond_the_bound(name, kind):
    """in the first block, in the last and in one in between: the final trunk activation moves by at least 10 F d(E, T), the logits by
    at least ten times their bound"""
    c = _case(name)
    T, E = c["T"], c["E", "native"]
    line_trunk = 10 * tl.F["trunk"] * tl.d(E["acts"][-1], T["acts"][-1])
    line_logits = 10 * tl.F["logits/native/rms"] * tl.d(E["logits"], T["logits"])
    for blk in (0, c["blocks"] // 2, c["blocks"] - 1):
        M = tl.forward(c["W"], c["s"], "truth", mutate=(kind, blk))
        dt, dl = tl.d(M["acts"][-1], T["acts"][-1]), tl.d(M["logits"], T["logits"])
        print("%s, %s in block %d: trunk moved by %.3g (%.0f x the bound), logits by %.3g (%.0f x), pi by %.3g, V by %.3g" % (
            name, kind, blk, dt, 10 * dt / line_trunk, dl, 10 * dl / line_logits, tl.d(M["pi"], T["pi"]), tl.d(M["V"], T["V"])))
        assert dt >= line_trunk and dl >= line_logits
        assert all(np.array_equal(M["acts"][i], T["acts"][i]) for i in range(1 + 2 * blk))   # nothing in front of the block moved


# ------------------------------------------------------------------------------------------------ the layer check

@pytest.mark.parametrize("name", NAMES)
def test_teacher_forced_check_on_the_reference_itself(name):
    """teacher_forced on E's own layers: nothing differs (here; the comment below).  On P's, a correct implementation by construction: no element is outside
    its interval, though a few are two ulp off by the plain measure (the function's docstring has why).  One element of a layer
    moved by one ulp: outside."""
    c = _case(name)
    h = lambda a: torch.from_numpy(a).half()
    worst = over = differ = 0
    for mode in ("E", "P"):
        acts = c[mode, "native"]["acts"]
        for i, (w, b) in enumerate(c["W"]["convs"]):
            x = c["s"] if i == 0 else h(acts[i - 1])
            res = h(acts[i - 2]) if i and i % 2 == 0 else None
            r = tl.teacher_forced(x, w, b, res, h(acts[i]))
            assert r["nan"] == 0 and r["outside"] == 0 and r["worst"] is None and r["bad"] == 0
            if mode == "E":   # nothing differs -- but for a sum that IS the midpoint of two fp16 values, which two orders of fp64 summation may round apart
                assert r["ulp"] <= 1 and r["share"] <= 1e-5
            else:
                assert r["ulp"] <= 2
                worst, over, differ = max(worst, r["ulp"]), over + r["over_one"], differ + (r["share"] > 0)
    print("%s: the fp32 proxy, layer by layer: worst %.3g ulp, %d elements more than one ulp off, %d layers differ" % (name, worst, over, differ))
    assert differ > 0
    i = 2 * c["blocks"]
    acts = c["E", "native"]["acts"]
    w, b = c["W"]["convs"][i]
    x, res, y = h(acts[i - 1]), h(acts[i - 2]), h(acts[i]).numpy().copy()
    at = np.unravel_index(int(y.argmax()), y.shape)
    r = tl.teacher_forced(x, w, b, res, torch.from_numpy(y))
    assert r["outside"] == 0 and r["worst"] is None
    y[at] = np.nextafter(y[at], np.float16(0))
    r = tl.teacher_forced(x, w, b, res, torch.from_numpy(y))
    # (the largest element is not next to a rounding boundary of its sum in any of the three nets: its interval is one value)
    assert r["outside"] == 1 and r["ulp"] == 1 and r["worst"]["at"] == tuple(int(v) for v in at) and r["worst"]["lo"] == r["worst"]["hi"]
