"""GPU: every inference route of the fp16 net against fp64, on a net whose outputs matter (tests/trained_like.py).

The kernels have batteries of their own (exact integers, halos, poisoned operands, ties, guards, bit-equality between routes); the
whole-net tests beside them run random-init nets, whose pi is nearly uniform and whose V is nearly 0 whatever the trunk does.  Here a
calibrated net (top-1 pi around 0.5, V over (-0.95, 0.95), half of every activation cut by its ReLU) runs through FusedInferenceNet
and NativeInferenceNet with each trunk kernel pinned on the instance, and is held to the CPU's fp64 truth T by way of E, the fp64
emulation of the documented roundings: d(Y, T) <= F d(E, T), with the factors F that test_trained_like_cpu.py derives from the
reference alone, and against which it shows a dropped skip, a skip from the wrong operand, a zeroed tap or K tile, a dropped bias and
taps shifted along a board edge to move the outputs by 28 to 1700 times their bound.  Every convolution of every route is also checked on
its own, teacher-forced on the fp16 input it was really given, which says which layer of which route broke."""
import copy
import ctypes as C

import numpy as np
import pytest

import conv_cases as cc
import trained_like as tl
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

# route -> (class, what is pinned ON THE INSTANCE, the trunk kernel every one of its 2 * blocks calls must then be, 256 channels only)
ROUTES = {
    "fused-algo0": ("FusedInferenceNet", dict(conv_algo=0), ("elfnet_conv3x3_f16", 0), False),
    "fused-algo1": ("FusedInferenceNet", dict(conv_algo=1), ("elfnet_conv3x3_f16", 1), True),
    "fused-small": ("FusedInferenceNet", dict(small_max_positions=1 << 20), ("elfnet_conv3x3_small_f16", None), False),
    "native": ("NativeInferenceNet", dict(), ("elfnet_conv3x3_f16", 0), False),
    "native-algo1": ("NativeInferenceNet", dict(conv_algo=1), ("elfnet_conv3x3_f16", 1), True),
    "native-small": ("NativeInferenceNet", dict(small_max_positions=1 << 20), ("elfnet_conv3x3_small_f16", None), False),
}
CASE_ROUTES = [(c[0], r) for c in tl.CASES for r in ROUTES if c[3] % 256 == 0 or not ROUTES[r][3]]


class _Calls:
    """the library with the trunk kernels' calls recorded as (name, algo)"""

    def __init__(self, L):
        self.L, self.trunk = L, []

    def __getattr__(self, name):
        f = getattr(self.L, name)
        if name not in ("elfnet_conv3x3_f16", "elfnet_conv3x3_small_f16"):
            return f

        def recorded(*a):
            self.trunk.append((name, a[-2] if name == "elfnet_conv3x3_f16" else None))
            return f(*a)
        return recorded


_cases, _runs = {}, {}


def _case(name):
    """the net of CASES[name] on the CPU and on the GPU, its feature rows, T and both head variants of E: computed once"""
    import torch
    if name not in _cases:
        _, n, blocks, dim, rows, scale, seed = next(c for c in tl.CASES if c[0] == name)
        s = tl.feature_rows(n, rows, tl.FEATURE_SEED)
        net = tl.build(n, blocks, dim, seed, s, scale)
        W = tl.weights(net)
        gpu = copy.deepcopy(net).cuda().to(memory_format=torch.channels_last)
        _cases[name] = dict(n=n, blocks=blocks, dim=dim, rows=rows, W=W, T=tl.forward(W, s, "truth"), net=gpu, s_cpu=s, E_from={},
                            s=s.cuda().contiguous(memory_format=torch.channels_last),
                            E={h: tl.forward(W, s, "emu", h) for h in ("native", "eager")})
    return _cases[name]


def _run(elf, name, route):
    """one call of the route with its `_conv` shadowed on the instance by a wrapper that clones (x, res, y) of every call.
    -> dict(inf, conv = its own `_conv`, out, rec = [(x, conv module, res, y)], acts = the activation after every trunk convolution, logits or None)"""
    import torch
    import elf_amd.net as N
    key = (name, route)
    if key in _runs:
        return _runs[key]
    c = _case(name)
    cls, pins, kernel, _ = ROUTES[route]
    inf = getattr(N, cls)(c["net"])
    for k, v in pins.items():
        setattr(inf, k, v)
    inf.L = _Calls(inf.L)
    rec, inner = [], inf._conv

    def recording(x, conv, res=None):
        y = inner(x, conv, res)
        rec.append((x.clone(), conv, None if res is None else res.clone(), y.clone()))
        return y
    inf._conv = recording
    out = inf({"s": c["s"]})
    torch.cuda.synchronize()
    assert inf.L.trunk == [kernel] * (2 * c["blocks"]), "%s ran %s" % (route, inf.L.trunk)
    native = cls == "NativeInferenceNet"
    assert len(rec) == 2 * c["blocks"] + (0 if native else 1)
    acts = ([rec[0][0]] if native else []) + [r[3] for r in rec]     # the native net's input convolution: the x of the first call
    logits = None
    if native:                                                        # elfnet_heads_f16 once more, with a logits buffer
        n, d, rows = c["n"], c["n"] * c["n"], c["rows"]
        nan = lambda *shape: torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)
        pi, v, logits = nan(rows, d + 1), nan(rows), nan(rows, d + 1)
        nb = inf.L.elfnet_heads_workspace(rows, n, n)
        ws = torch.empty((nb,), device="cuda", dtype=torch.uint8)
        inf.check(inf.L.elfnet_heads_f16(cc.ptr(acts[-1]), C.byref(inf.heads), rows, n, n, cc.ptr(pi), d + 1, cc.ptr(v), cc.ptr(logits),
                                         cc.ptr(ws), nb, cc.stream()))
        torch.cuda.synchronize()
        assert torch.equal(pi, out["pi"]) and torch.equal(v, out["V"])
    _runs[key] = dict(inf=inf, conv=inner, out=out, rec=rec, acts=acts, logits=logits, native=native)
    return _runs[key]


def _np(t):
    return t.double().cpu().numpy()


def _emu_from(c, first):
    """E of the eager-heads variant with the input convolution's output taken as the route returned it (one per distinct output)"""
    key = first.cpu().numpy().tobytes()
    if key not in c["E_from"]:
        c["E_from"][key] = tl.forward(c["W"], c["s_cpu"], "emu", "eager", first=first)
    return c["E_from"][key]


@pytest.mark.parametrize("name,route", CASE_ROUTES)
def test_route_against_fp64(elf, name, route):
    """One route, one case.  Figures of the first run on an MI355X are in DESIGN.md's parity section.
    1. trunk: d(Y, T) <= F d(E, T) for the activation after every block (the last is the final one), d(Y, E) <= F' d(E, T) for the final.
       For FusedInferenceNet the E of that last comparison (and of no other) starts from the input convolution's output as the route
       returned it: that convolution is MIOpen's, and on an MI355X its fp16 result is on the other side of a rounding boundary than the
       exact sum in 13 to 17 % of the elements, where this library's kernels are in 0.01 to 0.02 % (elf_amd/net.py's docstring); against
       the E of the exact input convolution its final activation is 1.13 to 1.24 d(E, T) away, by no fault of the trunk.
    2. every convolution teacher-forced (trained_like.teacher_forced has the criteria and their derivation): no NaN, and every element
       of one of this library's kernels inside the interval that the documented epilogue maps an fp32 accumulator's error onto: for
       most elements a single value, bit for bit.  "Within one fp16 ulp of the fp64 sequence" holds for all but 0 to 25 of a layer's
       83 000 to 740 000 elements, in these kernels and in the CPU test's fp32 proxy alike: a tie to even in the second rounding
       makes two ulp of a sum on the other side of a boundary, and where sum, bias and skip all cancel the accumulator's error is
       several ulp of a result of 1e-4.  MIOpen's input convolution in FusedInferenceNet is held to that plain measure, ties allowed.
    3. heads: rms and maximum of pi - T and V - T (and of the logits, for the native net) within their F of E's with the route's head
       variant; pi rows sum to 1 within 1e-5.
    4. where T's best move leads the second by more than 8 x max |E - T| of the logits, the route's argmax is T's; the same for the
       top-5 set where the gap behind it clears that line.  At least half the rows are checked."""
    c = _case(name)
    r = _run(elf, name, route)
    T, W, F = c["T"], c["W"], tl.F
    E = c["E"]["native" if r["native"] else "eager"]
    heads = "native" if r["native"] else "eager"
    acts = [_np(a) for a in r["acts"]]
    failures = []

    def hold(what, got, bound):
        if not got <= bound:          # a NaN fails
            failures.append("%s: %.4g > %.4g" % (what, got, bound))

    # 1
    ratio_trunk = 0.0
    for i in range(2, len(acts), 2):
        det = tl.d(E["acts"][i], T["acts"][i])
        ratio_trunk = max(ratio_trunk, tl.d(acts[i], T["acts"][i]) / det)
        hold("trunk after block %d, d(Y,T)" % (i // 2 - 1), tl.d(acts[i], T["acts"][i]), F["trunk"] * det)
    det = tl.d(E["acts"][-1], T["acts"][-1])
    E_own = E if r["native"] else _emu_from(c, r["acts"][0])
    hold("final activation, d(Y,E)", tl.d(acts[-1], E_own["acts"][-1]), F["trunk_emu"] * det)
    # 2
    worst = share = over = far = 0
    layers = [(c["s"], c["net"].init_conv[0], None, r["acts"][0])] + r["rec"] if r["native"] else r["rec"]
    assert len(layers) == len(W["convs"])
    for i, (x, conv, res, y) in enumerate(layers):
        tf = tl.teacher_forced(x, conv.weight, conv.bias, res, y)
        ours = r["native"] or i > 0       # FusedInferenceNet's first convolution is MIOpen's
        worst, share, over, far = max(worst, tf["ulp"]), max(share, tf["share"]), over + tf["over_one"], far + (tf["outside"] if ours else 0)
        if tf["nan"] or (tf["outside"] if ours else tf["bad"] or not tf["ulp"] <= 2):
            failures.append("convolution %d on its own: %s" % (i, tf))
    # 3
    pi, v = _np(r["out"]["pi"]), _np(r["out"]["V"])
    got = dict(pi=pi, V=v)
    if r["native"]:
        got["logits"] = _np(r["logits"])
    ratios = {}
    for q, y in got.items():
        ratios[q] = tl.d(y, T[q]) / tl.d(E[q], T[q])
        hold("d(%s, T)" % q, tl.d(y, T[q]), F["%s/%s/rms" % (q, heads)] * tl.d(E[q], T[q]))
        hold("max |%s - T|" % q, tl.dmax(y, T[q]), F["%s/%s/max" % (q, heads)] * tl.dmax(E[q], T[q]))
    hold("max |sum pi - 1|", float(np.abs(pi.sum(axis=1) - 1).max()), 1e-5)
    # 4
    checked = {}
    for top in (1, 5):
        ok, want = tl.decided_rows(T, E, top)
        checked[top] = len(ok)
        if not np.array_equal(tl.top_sets(pi, top)[ok], want[ok]):
            failures.append("top-%d differs from T's in a decided row" % top)
    if 2 * checked[1] < c["rows"]:
        failures.append("only %d of %d rows have a decided best move" % (checked[1], c["rows"]))
    print("%s %s: d(E,T) trunk %.6g;  d(Y,T)/d(E,T): trunk %.3f  d(Y,E)/d(E,T) %.3f (E of the exact input convolution: %.3f)  %s;  teacher-forced: worst %.3g ulp, %d elements "
          "over one ulp, %d outside their interval, at most %.3g of a layer differ;  argmax checked in %d, top-5 in %d of %d rows"
          % (name, route, det, ratio_trunk, tl.d(acts[-1], E_own["acts"][-1]) / det, tl.d(acts[-1], E["acts"][-1]) / det, "  ".join("%s %.3f" % (q, ratios[q]) for q in sorted(ratios)),
             worst, over, far, share, checked[1], checked[5], c["rows"]))
    assert not failures, "\n".join(failures)


def _eager_heads_repeat(net, h):
    """do the head ops of FusedInferenceNet.__call__ return the same bits three times for the one activation h"""
    import torch
    outs = []
    with torch.no_grad():
        for _ in range(3):
            pi = net.pi_linear(net.pi_final_conv(h).reshape(-1, 2 * net.d))
            v = net.value_linear2(torch.relu(net.value_linear1(net.value_final_conv(h).reshape(-1, net.d))))
            outs.append((pi, v))
    torch.cuda.synchronize()
    differ = [int((a != outs[0][0]).sum()) + int((b != outs[0][1]).sum()) for a, b in outs[1:]]
    print("the eager head ops, three times on one activation: %s logits or values differ from the first call's" % differ)
    return not any(differ)


@pytest.mark.parametrize("name", [c[0] for c in tl.CASES])
def test_routes_agree(elf, name):
    """The activation after every trunk convolution is the same bits in every FusedInferenceNet route, and in every
    NativeInferenceNet route; so are pi and V -- for FusedInferenceNet where its head ops, which are PyTorch's, return the same bits
    twice for one activation.  They do not everywhere: at 19 x 19 x 256 channels and 8 rows MIOpen's 1 x 1 policy head convolution
    returned other bits call after call in every run of this test on an MI355X (about 1600 of its 5776 outputs, on an input that was
    the same bits; the value head and the Linear layers repeated), so there equal trunks give a pi between 1.06 and 1.96 d(E, T)
    from T.  The test
    repeats the head ops on one activation first and says what it found.  Between the two classes the input convolution is another kernel (MIOpen's against
    elfnet_conv3x3_in_f16), so the trunks are tied by running a fused route's own `_conv` chain on the native net's input activation:
    the final activation is the native routes' bit for bit, here with a trained net's sparsity and range.  Where the two input
    convolutions happen to agree, all final activations are compared directly.
    The eager fp16 PyTorch net runs beside them as a yardstick: printed, nothing asserted."""
    import torch
    c = _case(name)
    routes = [r for n, r in CASE_ROUTES if n == name]
    runs = {r: _run(elf, name, r) for r in routes}
    for family in (True, False):
        fam = [r for r in routes if runs[r]["native"] == family]
        assert len(fam) == (3 if c["dim"] % 256 == 0 else 2)
        first = runs[fam[0]]
        assert not any(bool(torch.isnan(a).any()) for a in first["acts"])
        for r in fam[1:]:
            for i, (a, b) in enumerate(zip(first["acts"], runs[r]["acts"])):
                assert torch.equal(a, b), "%s and %s differ behind trunk convolution %d" % (fam[0], r, i)
            same = torch.equal(first["out"]["pi"], runs[r]["out"]["pi"]) and torch.equal(first["out"]["V"], runs[r]["out"]["V"])
            assert same or (not family and not _eager_heads_repeat(c["net"], first["acts"][-1])), "%s and %s differ in pi or V" % (fam[0], r)
    native, fused = runs["native"], runs["fused-algo0"]
    h = native["acts"][0]
    for lo, up in fused["inf"].blocks:
        h = fused["conv"](fused["conv"](h, lo), up, res=h)
    torch.cuda.synchronize()
    assert torch.equal(h, native["acts"][-1])
    same_in = torch.equal(native["acts"][0], fused["acts"][0])
    print("%s: the two input convolutions differ in %d of %d elements" % (name, int((native["acts"][0] != fused["acts"][0]).sum()), h.numel()))
    if same_in:
        assert torch.equal(fused["acts"][-1], native["acts"][-1])
    eager = c["net"]({"s": c["s"]})
    torch.cuda.synchronize()
    T, E = c["T"], c["E"]["eager"]
    print("%s: eager fp16 net: d(Y,T)/d(E,T) pi %.3f  V %.3f;  fused pi %.3f  V %.3f" % (
        name, tl.d(_np(eager["pi"]), T["pi"]) / tl.d(E["pi"], T["pi"]), tl.d(_np(eager["V"]), T["V"]) / tl.d(E["V"], T["V"]),
        tl.d(_np(fused["out"]["pi"]), T["pi"]) / tl.d(E["pi"], T["pi"]), tl.d(_np(fused["out"]["V"]), T["V"]) / tl.d(E["V"], T["V"])))
