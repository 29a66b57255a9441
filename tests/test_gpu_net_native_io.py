"""GPU: the two ends of the native fp16 net (elf_amd/csrc/net_io.hip) and NativeInferenceNet on top of them.

The method is test_gpu_net_conv_native.py's: inputs whose result is exact -- small integers and small multiples of powers of two, so
every partial sum is a number fp32 holds exactly in any summation order -- make any differing element a layout, halo, tail or
flattening bug and never rounding.  Real feature rows and random weights then bound the rounding itself against fp64, with the
MIOpen pair / the eager FusedInferenceNet measured in the same test as the yardstick."""
import copy
import ctypes as C

import numpy as np
import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

INTS = dict(res=False, limit=288)      # cc.int_case without res: |sum| <= 9 * 32 = 288, far below 2048: exact in fp32 and in fp16


def _seed(rows, h, wd, c, k):
    return 911 + rows + 1000 * h + c + 7 * k


# ------------------------------------------------------------------------------------------------ input conv, exact

@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,n,c,k", [(3, 19, 18, 256),     # 1083 positions: a tail tile
                                        (1, 19, 18, 256),
                                        (5, 9, 18, 64),       # tiles straddle boards
                                        (2, 9, 2, 32),        # the smallest c and k
                                        (3, 9, 32, 64),       # the largest c: the 18-step instance
                                        (64, 9, 18, 32),      # 5184 positions = 81 tiles of 64: several tiles, no remainder
                                        (2, 9, 18, 288),      # two workgroups along k, the second with one wave's channels
                                        (410, 9, 18, 32)])    # 519 tiles: more than workgroups, the tile loop goes round
def test_input_conv_exact_integers(elf, rows, n, c, k, relu):
    """equality with the nine-tap fp32 form; y is prefilled with NaN, and one guard row of NaN behind y's last row stays NaN"""
    import torch
    d = cc.int_case(_seed(rows, n, n, c, k), rows, n, n, c, k, **INTS)
    ref = d["conv"] + d["b"].float()
    if relu:
        ref = torch.relu(ref)
    buf, y = cc.guarded(rows, n, n, k)
    assert cc.conv_in(elf.lib(), d["x"], d["w"], d["b"], y, rows, n, n, c, k, relu) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
    print("rows %d n %d c %d k %d relu %d: %d of %d differ" % (rows, n, c, k, relu, bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("n", [19, 9])
def test_input_conv_all_ones_halo(elf, n):
    """x = 1, w = 1, bias = 0: every output is C x the number of on-board taps: 4 C at corners, 6 C on edges, 9 C inside"""
    import torch
    rows, c, k = 2, 18, 64
    x = torch.ones((rows, n, n, c), device="cuda", dtype=torch.float16)
    w = torch.ones((k, 3, 3, c), device="cuda", dtype=torch.float16)
    b = torch.zeros((k,), device="cuda", dtype=torch.float16)
    y = torch.full((rows, n, n, k), float("nan"), device="cuda", dtype=torch.float16)
    assert cc.conv_in(elf.lib(), x, w, b, y, rows, n, n, c, k, 0) == 0
    torch.cuda.synchronize()
    i = torch.arange(n, device="cuda")
    on = 3 - ((i == 0) | (i == n - 1)).long()           # taps on the board along one axis
    want = (c * on[:, None] * on[None, :]).float()      # [n, n]
    assert want[0, 0] == 4 * c and want[0, 1] == 6 * c and want[1, 1] == 9 * c
    assert bool((y.float() == want[None, :, :, None]).all())


# ------------------------------------------------------------------------------------------------ real feature rows

_feat = {}


def _feature_rows(elf, n, rows):
    """`rows` ELFGO_FEAT_F16_NHWC rows (fp16 [rows,18,n,n], channels_last) of random positions, every board under another symmetry"""
    import torch
    key = (n, rows)
    if key not in _feat:
        rng = np.random.RandomState(5 + n + rows)
        eng = elf.GoEngine(n, rows, 0)
        stones = rng.choice(np.array([0, 1, 2], np.uint8), size=(rows, n * n), p=[0.6, 0.2, 0.2])
        ok = eng.setup(stones, next_player=[1 + (i & 1) for i in range(rows)]).cpu().numpy()
        assert ok.sum() >= rows // 2          # a refused row (a group without a liberty) stays an empty board, which is a position too
        s = eng.extract_agz(d4=[i % 8 for i in range(rows)], fmt="f16_nhwc").clone()
        torch.cuda.synchronize()
        eng.close()
        assert s.dtype == torch.float16 and tuple(s.shape) == (rows, 18, n, n) and float(s.float().sum()) > 0
        _feat[key] = s
    return _feat[key]


def _real_case(elf):
    import torch
    rows, n, c, k = 8, 19, 18, 256
    s = _feature_rows(elf, n, rows)
    x = s.permute(0, 2, 3, 1)                     # the NHWC memory as it lies
    assert x.is_contiguous()
    g = torch.Generator(device="cuda").manual_seed(31)
    w = (torch.randn((k, 3, 3, c), device="cuda", generator=g) * (9 * c) ** -0.5).half()
    b = torch.randn((k,), device="cuda", generator=g).half()
    return rows, n, c, k, s, x, w, b


def test_input_conv_real_feature_rows_against_fp64(elf):
    """Binary feature planes, random fp16 weights.  The truth is the fp64 convolution pushed through the kernel's two roundings
    (fp16, + bias and ReLU in fp32, fp16; numpy converts fp64 -> fp16 in one step).  Every element within one fp16 ulp, and the share
    of elements that differ at all at most twice that of F.conv2d without bias + elfnet_bias_act_f16, measured here.
    The ulp is that of the larger of the rounded convolution and the result: an fp32 accumulator that lands on the other side of a
    rounding boundary moves the first rounding by one ulp OF THE CONVOLUTION VALUE, and the bias may then cancel most of it, so the
    result's own (smaller) ulp is not the unit of that step."""
    import torch
    L = elf.lib()
    rows, n, c, k, s, x, w, b = _real_case(elf)
    conv64 = cc.conv_fp32(x.double(), w.double()).cpu().numpy()
    r1 = conv64.astype(np.float16).astype(np.float32)
    ref = np.maximum(r1 + b.cpu().numpy().astype(np.float32)[None, None, None, :], np.float32(0)).astype(np.float16)
    y = torch.full((rows, n, n, k), float("nan"), device="cuda", dtype=torch.float16)
    assert cc.conv_in(L, x, w, b, y, rows, n, n, c, k, 1) == 0
    pair = torch.nn.functional.conv2d(s, w.permute(0, 3, 1, 2), None, 1, 1)
    assert pair.is_contiguous(memory_format=torch.channels_last)
    assert L.elfnet_bias_act_f16(cc.ptr(pair), cc.ptr(b), None, rows * n * n, k, 1, cc.stream()) == 0
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    got_pair = pair.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    ulp = np.maximum(np.maximum(np.spacing(np.abs(ref)), np.spacing(np.abs(got))), np.spacing(np.abs(r1.astype(np.float16)))).astype(np.float32)
    err = np.abs(got.astype(np.float32) - ref.astype(np.float32))
    share = float((got != ref).mean())
    share_pair = float((got_pair != ref).mean())
    print("share of elements that differ from the fp64 sequence: native %.3e, conv2d + bias_act %.3e; worst native error %.3g ulp"
          % (share, share_pair, float((err / ulp).max())))
    assert not np.isnan(got).any()
    assert bool((err <= ulp).all())
    assert share <= 2 * share_pair


# ------------------------------------------------------------------------------------------------ heads

def _upload(a):
    """name -> fp16 device tensor of every array in `a` (all of them exactly representable)"""
    import torch
    out = {}
    for nm, v in a.items():
        h = v.astype(np.float16)
        assert np.array_equal(h.astype(np.float64), v), nm
        out[nm] = torch.from_numpy(h).cuda()
    return out


def _heads_ref(a, rows, d):
    """fp64: logits [rows, d+1], pi, V"""
    act = a["act"].reshape(rows, d, -1)
    p = np.maximum(act @ a["pconv_w"].T + a["pconv_b"], 0)                  # [rows, d, 2]
    flat = p.transpose(0, 2, 1).reshape(rows, 2 * d)                       # torch's flattening of [B,2,H,W]: c * d + pos
    logits = flat @ a["pi_w"].T + a["pi_b"]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    pi = e / e.sum(axis=1, keepdims=True)
    v0 = np.maximum(act @ a["vconv_w"].T + a["vconv_b"], 0)[:, :, 0]        # [rows, d]
    v1 = np.maximum(v0 @ a["v1_w"].T + a["v1_b"], 0)
    pre = v1 @ a["v2_w"].T + a["v2_b"]
    return logits, pi, np.tanh(pre)[:, 0], pre[:, 0]


_hexact = {}


def _heads_exact_case(rows, n, ch):
    """act in {0,1,2} (1/2, 1/4, 1/4); head-conv weights in {-1,0,1} with 3/4 zeros, integer biases in [-2,2]; pi_w, v1_w in
    {-1,0,1}/8 with 7/8 zeros, their biases multiples of 1/8; v2_w in {-1,1}/32 (scaled up from /64 so that the value leaves tanh's
    linear part).  Every partial sum is a small multiple of 1/64: exact in fp32 in any order."""
    key = (rows, n, ch)
    if key not in _hexact:
        rng = np.random.RandomState(1000 * rows + 10 * n + ch)
        d, vh = n * n, 256
        tern = lambda shape, pz: rng.choice([-1.0, 0.0, 1.0], size=shape, p=[(1 - pz) / 2, pz, (1 - pz) / 2])
        a = dict(act=rng.choice([0.0, 1.0, 2.0], size=(rows, n, n, ch), p=[0.5, 0.25, 0.25]),
                 pconv_w=tern((2, ch), 0.75), pconv_b=rng.randint(-2, 3, size=(2,)).astype(np.float64),
                 vconv_w=tern((1, ch), 0.75), vconv_b=rng.randint(-2, 3, size=(1,)).astype(np.float64),
                 pi_w=tern((d + 1, 2 * d), 0.875) / 8, pi_b=rng.randint(-8, 9, size=(d + 1,)) / 8.0,
                 v1_w=tern((vh, d), 0.875) / 8, v1_b=rng.randint(-8, 9, size=(vh,)) / 8.0,
                 v2_w=tern((1, vh), 0.0) / 32, v2_b=rng.randint(-2, 3, size=(1,)) / 8.0)
        logits, pi, v, pre = _heads_ref(a, rows, d)
        # the reference is not degenerate: a softmax with mass on many entries, a value off tanh's flat ends
        assert ((pi > 1e-6).sum(axis=1) >= 10).all() and (np.abs(v) < 0.999).all()
        assert np.array_equal(logits.astype(np.float32).astype(np.float64), logits) and np.array_equal(pre.astype(np.float32), pre)
        _hexact[key] = dict(a=a, t=_upload(a), logits=logits, pi=pi, v=v, vh=vh)
    return _hexact[key]


def _run_heads(L, t, ch, vh, rows, n, stride=None, want_logits=True):
    """-> (status, pi buffer [rows, stride], value buffer [rows + 1], logits buffer or None); all prefilled with NaN"""
    import torch
    d = n * n
    stride = d + 1 if stride is None else stride
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)
    pi, value, logits = nan(rows, stride), nan(rows + 1), nan(rows, stride) if want_logits else None
    nb = L.elfnet_heads_workspace(rows, n, n)
    ws = torch.empty((nb,), device="cuda", dtype=torch.uint8)
    hd = cc.heads_struct(t, ch, vh)
    rc = L.elfnet_heads_f16(cc.ptr(t["act"]), C.byref(hd), rows, n, n, cc.ptr(pi), stride, cc.ptr(value), cc.ptr(logits), cc.ptr(ws), nb,
                            cc.stream())
    torch.cuda.synchronize()
    return rc, pi, value, logits


@pytest.mark.parametrize("rows,n,ch,pad,want_logits", [(1, 19, 256, 0, True),
                                                        (3, 19, 256, 6, True),     # pi_stride = d + 1 + 6
                                                        (5, 9, 64, 0, False),      # logits = NULL
                                                        (17, 9, 64, 0, True),      # more rows than one workgroup's share
                                                        (515, 9, 128, 0, True),    # two rows per workgroup, the last one half full
                                                        (2053, 9, 8, 0, True),     # eight rows per workgroup; the smallest C
                                                        (2, 9, 512, 0, True)])     # more 16-B chunks per position than lanes in a group
def test_heads_exact(elf, rows, n, ch, pad, want_logits):
    """logits bit-equal to the fp64 reference; pi within relative 1e-4 of the fp64 softmax (a 4-ulp expf, a (d+1)-term fp32 sum and
    one division: about 2.3e-5); |sum pi - 1| <= 1e-5; V within 2^-20 of fp64 tanh (a 4-ulp tanhf and the final rounding).  The
    padding of a strided pi / logits row and the element behind value stay NaN."""
    cs = _heads_exact_case(rows, n, ch)
    d = n * n
    rc, pi, value, logits = _run_heads(elf.lib(), cs["t"], ch, cs["vh"], rows, n, d + 1 + pad, want_logits)
    assert rc == 0
    pi, value = pi.cpu().numpy(), value.cpu().numpy()
    if want_logits:
        lg = logits.cpu().numpy()
        bad = int((lg[:, :d + 1] != cs["logits"].astype(np.float32)).sum())
        print("logits: %d of %d differ" % (bad, rows * (d + 1)))
        assert bad == 0
        assert np.isnan(lg[:, d + 1:]).all()
    rel = np.abs(pi[:, :d + 1].astype(np.float64) - cs["pi"]) / cs["pi"]
    verr = np.abs(value[:rows].astype(np.float64) - cs["v"])
    print("pi: max relative error %.3g, max |sum - 1| %.3g; V: max error %.3g (2^-20 = %.3g)"
          % (rel.max(), np.abs(pi[:, :d + 1].astype(np.float64).sum(axis=1) - 1).max(), verr.max(), 2.0 ** -20))
    assert not np.isnan(pi[:, :d + 1]).any() and not np.isnan(value[:rows]).any()
    assert rel.max() <= 1e-4
    assert np.abs(pi[:, :d + 1].astype(np.float64).sum(axis=1) - 1).max() <= 1e-5
    assert verr.max() <= 2.0 ** -20
    assert np.isnan(pi[:, d + 1:]).all() and np.isnan(value[rows])


@pytest.mark.parametrize("n,ch,row0,pos0", [(9, 64, 1, 23), (19, 256, 0, 200)])
def test_heads_policy_flattening_is_channel_major(elf, n, ch, row0, pos0):
    """only p[1][pos0] of one row is non-zero (= 1): the logits of that row are exactly column d + pos0 of pi_w (pi_b = 0), the
    other rows' are 0.  A pos * 2 + c flattening would pick column 2 pos0 + 1."""
    rng = np.random.RandomState(n + pos0)
    rows, d, vh = 2, n * n, 8
    a = dict(act=np.zeros((rows, n, n, ch)), pconv_w=np.zeros((2, ch)), pconv_b=np.zeros(2), vconv_w=np.zeros((1, ch)),
             vconv_b=np.zeros(1), pi_w=rng.randint(-64, 65, size=(d + 1, 2 * d)) / 8.0, pi_b=np.zeros(d + 1), v1_w=np.zeros((vh, d)),
             v1_b=np.zeros(vh), v2_w=np.zeros((1, vh)), v2_b=np.zeros(1))
    a["act"].reshape(rows, d, ch)[row0, pos0, 5] = 1.0
    a["pconv_w"][1, 5] = 1.0
    assert d + pos0 != 2 * pos0 + 1 and not np.array_equal(a["pi_w"][:, d + pos0], a["pi_w"][:, 2 * pos0 + 1])
    rc, pi, value, logits = _run_heads(elf.lib(), _upload(a), ch, vh, rows, n)
    assert rc == 0
    lg = logits.cpu().numpy()
    assert np.array_equal(lg[row0], a["pi_w"][:, d + pos0].astype(np.float32))
    assert np.array_equal(lg[1 - row0], np.zeros(d + 1, np.float32))
    assert np.array_equal(value.cpu().numpy()[:rows], np.zeros(rows, np.float32))


# ------------------------------------------------------------------------------------------------ determinism

def test_repeated_launches_return_the_same_bits(elf):
    """twenty launches of each kernel on random inputs return the bits of the first: no atomics, no order that depends on timing"""
    import torch
    L = elf.lib()
    rows, n, c, k, s, x, w, b = _real_case(elf)
    first = None
    for i in range(20):
        y = torch.full((rows, n, n, k), float("nan"), device="cuda", dtype=torch.float16)
        assert cc.conv_in(L, x, w, b, y, rows, n, n, c, k, 1) == 0
        torch.cuda.synchronize()
        if first is None:
            first = y
            assert not bool(torch.isnan(y).any())
        else:
            assert torch.equal(y, first), "input conv: launch %d differs from the first" % i
    d, vh = n * n, 256
    g = torch.Generator(device="cuda").manual_seed(77)
    rn = lambda shape, scale: (torch.randn(shape, device="cuda", generator=g) * scale).half()
    t = dict(act=torch.relu(rn((rows, n, n, k), 1.0)), pconv_w=rn((2, k), k ** -0.5), pconv_b=rn((2,), 0.1), vconv_w=rn((1, k), k ** -0.5),
             vconv_b=rn((1,), 0.1), pi_w=rn((d + 1, 2 * d), (2 * d) ** -0.5), pi_b=rn((d + 1,), 0.1), v1_w=rn((vh, d), d ** -0.5),
             v1_b=rn((vh,), 0.1), v2_w=rn((1, vh), vh ** -0.5), v2_b=rn((1,), 0.1))
    first = None
    for i in range(20):
        rc, pi, value, logits = _run_heads(L, t, k, vh, rows, n)
        assert rc == 0
        if first is None:
            first = (pi, value[:rows], logits)
            assert not any(bool(torch.isnan(v).any()) for v in first)
        else:
            assert torch.equal(pi, first[0]) and torch.equal(value[:rows], first[1]) and torch.equal(logits, first[2]), \
                "heads: launch %d differs from the first" % i


# ------------------------------------------------------------------------------------------------ NativeInferenceNet

_nets = {}


def _net_case(elf, n, blocks, dim, rows):
    """(net, feature rows, fp64 truth of the same fp16 weights on the CPU: pi [rows, d+1], V [rows])"""
    import torch
    from elf_amd.net import make_net
    key = (n, blocks, dim, rows)
    if key not in _nets:
        net = make_net(board_size=n, num_block=blocks, dim=dim, fold_bn=True)
        s = _feature_rows(elf, n, rows)
        ref = copy.deepcopy(net).cpu().double().to(memory_format=torch.contiguous_format)
        with torch.no_grad():
            h = ref.resnet(ref.init_conv(s.cpu().double().contiguous()))
            pi = torch.softmax(ref.pi_linear(ref.pi_final_conv(h).reshape(-1, 2 * ref.d)), dim=1)
            v = torch.relu(ref.value_linear1(ref.value_final_conv(h).reshape(-1, ref.d)))
            v = torch.tanh(ref.value_linear2(v)).reshape(-1)
        _nets[key] = (net, s, pi.numpy(), v.numpy())
    return _nets[key]


@pytest.mark.parametrize("n,blocks,dim,rows", [(9, 2, 64, 8), (19, 1, 256, 3)])
def test_native_net_is_no_less_accurate_than_the_fused_net(elf, monkeypatch, n, blocks, dim, rows):
    """max |pi - truth| and max |V - truth| of NativeInferenceNet at most 2 x FusedInferenceNet's on the same rows (fewer roundings
    must not be less accurate; the factor is for the maximum over a few thousand values) -- and the native call runs with
    F.conv2d, F.linear, torch.softmax and torch.tanh made to raise."""
    import torch
    from elf_amd.net import FusedInferenceNet, NativeInferenceNet
    net, s, pi64, v64 = _net_case(elf, n, blocks, dim, rows)
    fused = FusedInferenceNet(net)({"s": s})
    native_net = NativeInferenceNet(net)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError("NativeInferenceNet called " + name)
        return f
    with monkeypatch.context() as m:
        m.setattr(torch.nn.functional, "conv2d", refuse("F.conv2d"))
        m.setattr(torch.nn.functional, "linear", refuse("F.linear"))
        m.setattr(torch, "softmax", refuse("torch.softmax"))
        m.setattr(torch, "tanh", refuse("torch.tanh"))
        native = native_net({"s": s})
        torch.cuda.synchronize()
    err = lambda o: (float(np.abs(o["pi"].double().cpu().numpy() - pi64).max()), float(np.abs(o["V"].double().cpu().numpy() - v64).max()))
    (pn, vn), (pf, vf) = err(native), err(fused)
    print("max |pi - fp64|: native %.3e fused %.3e;  max |V - fp64|: native %.3e fused %.3e" % (pn, pf, vn, vf))
    assert native["pi"].dtype == torch.float32 and tuple(native["pi"].shape) == (rows, n * n + 1) and tuple(native["V"].shape) == (rows,)
    assert pn <= 2 * pf
    assert vn <= 2 * vf


def test_native_net_refuses_what_it_cannot_take_completely(elf):
    import torch
    from elf_amd.net import NativeInferenceNet, make_net
    with pytest.raises(ValueError):
        NativeInferenceNet(make_net(board_size=9, num_block=1, dim=64, dtype=torch.bfloat16, fold_bn=True))
    with pytest.raises(ValueError):
        NativeInferenceNet(make_net(board_size=9, num_block=1, dim=64, fold_bn=False))


def test_native_net_replays_from_a_graph_to_the_same_bits(elf):
    """GraphedNet(NativeInferenceNet): a straight-line graph of kernel launches only; the replay returns the eager call's bits"""
    import torch
    from elf_amd.net import GraphedNet, NativeInferenceNet
    net, s, _, _ = _net_case(elf, 9, 2, 64, 8)
    native = NativeInferenceNet(net)
    eager = native({"s": s})
    torch.cuda.synchronize()
    s_static = s.clone(memory_format=torch.preserve_format)
    graphed = GraphedNet(native, s_static)
    out = graphed()
    torch.cuda.synchronize()
    assert torch.equal(out["pi"], eager["pi"]) and torch.equal(out["V"], eager["V"])
    # chunked_forward: slices of 3 rows (the last one shorter) give the rows of the one call
    from elf_amd.net import chunked_forward
    ch = chunked_forward(native, s, 3)
    torch.cuda.synchronize()
    assert torch.equal(ch["pi"], eager["pi"]) and torch.equal(ch["V"], eager["V"])


def test_native_net_serves_a_search(elf):
    """A 9 x 9 search of 32 rollouts per move through begin_step / end_step with pi and V as NativeInferenceNet returns them (fp32,
    no cast): the node records keep their invariants and every logged search's visit counts add up."""
    import torch
    from elf_amd.net import NativeInferenceNet
    net, _, _, _ = _net_case(elf, 9, 2, 64, 8)
    native = NativeInferenceNet(net)
    sp = elf.SelfPlay(board_size=9, num_games=2, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, feature_format="f16_nhwc",
                      seed=5, log_searches=4)
    steps = 0
    while sp.stats()["logged"] < 4 and steps < 200:
        rows = sp.begin_step()
        if rows:
            o = native({"s": sp.s[:rows]})
            assert o["pi"].dtype == torch.float32 and o["pi"].is_contiguous() and o["V"].dtype == torch.float32
            sp.end_step(o["pi"], o["V"])
        else:
            sp.end_step(None, None)
        steps += 1
    assert sp.stats()["logged"] >= 4
    assert sp.validate_trees()[0] == 0
    rec, coord, visits, prior, reward = sp.search_log()
    for i in range(4):
        ne = rec[i].n_edges
        assert ne > 0 and rec[i].total_visits > 0 and int(visits[i, :ne].sum()) == rec[i].total_visits
        assert np.isfinite(prior[i, :ne]).all() and np.isfinite(reward[i, :ne]).all()
    sp.close()
