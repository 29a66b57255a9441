"""A net whose outputs matter, and what it computes, on the CPU in fp64.  A helper of test_trained_like_cpu.py and
test_gpu_net_trained_like.py, not a test: pure torch-on-CPU and numpy, deterministic from a seed.

make_net leaves BatchNorm at identity and the heads at PyTorch's default init: pi is nearly uniform, V nearly 0, and almost nothing in
the trunk can move them.  `build` returns a PolicyValueNet with randomised, folded BatchNorms and a data-dependent calibration, so
that activations have an rms around 1, the ReLUs cut about half, pi has a clear top move and V spreads over (-1, 1): a dropped skip
connection or a tap read one cell off moves the outputs by far more than fp16 rounding does (test_trained_like_cpu.py measures it).

Three forwards of the same fp16 weights, each returning the activation after every trunk convolution, the logits, pi, the pre-tanh
value and V as fp64 numpy arrays:
    truth  T  no rounding anywhere
    emu    E  the rounding contract the kernels document (elf_amd/csrc/net_conv3x3.hip, net_conv3x3_small.hip, net_io.hip): the exact
              sum of a convolution is rounded to fp16; bias and skip are added in fp32, max(., 0); one rounding to fp16.  The heads:
              "native": elfnet_heads_f16, fp32 from the trunk activation to pi / V, no rounding to fp16 in between.
              "eager":  the fp16 PyTorch ops FusedInferenceNet runs behind its trunk.  Written out here, each one computing in fp32
                        and rounding its result to fp16: the 1x1 head convolution (sum -> fp16), its bias add (-> fp16), ReLU;
                        pi_linear (sum + bias -> fp16), softmax in fp32 on those fp16 logits; value_linear1 (sum + bias -> fp16),
                        ReLU; value_linear2 (sum + bias -> fp16); tanh (-> fp16).
    proxy  P  emu's rounding points with every sum taken in fp32 by this machine's F.conv2d / F.linear: a correct kernel whose only
              freedom is its summation order.

With d(A, B) the rms of A - B over all elements, a route Y under test is held to d(Y, T) <= F * d(E, T).  The factors F are derived
from the reference alone, by test_trained_like_cpu.py::test_factors_are_derived_from_the_reference: 1.5 x the largest d(P, T) / d(E, T)
over 8 seeds of each of CASES (the margin: a kernel's summation order is another sample of the same rounding noise than the proxy's).
"""
import numpy as np
import torch
import torch.nn.functional as Fn

# (name, board, blocks, channels, rows, scale, seed of the net): the shapes the GPU test runs; the smallest that still reach every route.
# 19 x 19 x 8 rows = 2888 positions: a partial last 256-position tile, one channel column for algo 1, 46 x 4 tiles for the small kernel.
# A power-of-two scale is exact in fp16, so the scale-32 net is a net of scale 1 seen through larger exponents (accumulators in the
# thousands, the coarse end of fp16's spacing); it has a seed of its own, so that it is not the first case over again.
CASES = (("9x9", 9, 6, 64, 16, 1.0, 11),
         ("9x9-scale32", 9, 6, 64, 16, 32.0, 31),
         ("19x19", 19, 3, 256, 8, 1.0, 11))
FEATURE_SEED = 7
FACTOR_SEEDS = 8       # the CPU test derives the factors from the 8 seeds from each case's own on

# F[quantity] = 1.5 x the largest ratio over CASES x 8 seeds, rounded up to two decimals; RATIOS_SEEN has the (smallest, largest)
# ratio measured.  "quantity/heads/rms" is d(P, T) / d(E, T), "/max" the same of max |. - T|; "trunk" is the largest of the ratios of
# the activations after every block, "trunk_emu" is d(P, E) / d(E, T) of the final activation.  Both are checked by
# test_trained_like_cpu.py: on another CPU the proxy sums in another order and its ratios differ, so that test holds the proxy to F and
# F to within 1.5 x of its own derivation, not the recorded ratios to the digit.  (V has 8 or 16 elements per case: it spreads most.)
RATIOS_SEEN = {
    "V/eager/max": (0.517, 2.166),
    "V/eager/rms": (0.664, 1.940),
    "V/native/max": (0.482, 1.702),
    "V/native/rms": (0.668, 1.547),
    "logits/eager/max": (0.823, 1.360),
    "logits/eager/rms": (0.955, 1.038),
    "logits/native/max": (0.830, 1.180),
    "logits/native/rms": (0.969, 1.048),
    "pi/eager/max": (0.497, 1.738),
    "pi/eager/rms": (0.639, 1.497),
    "pi/native/max": (0.735, 1.423),
    "pi/native/rms": (0.786, 1.326),
    "trunk": (1.000, 1.005),
    "trunk_emu": (0.445, 0.693),
}
F = {
    "V/eager/max": 3.25,
    "V/eager/rms": 2.91,
    "V/native/max": 2.56,
    "V/native/rms": 2.33,
    "logits/eager/max": 2.04,
    "logits/eager/rms": 1.56,
    "logits/native/max": 1.77,
    "logits/native/rms": 1.58,
    "pi/eager/max": 2.61,
    "pi/eager/rms": 2.25,
    "pi/native/max": 2.14,
    "pi/native/rms": 1.99,
    "trunk": 1.51,
    "trunk_emu": 1.04,
}

MUTATIONS = ("skip_dropped", "skip_from_lower", "tap_zeroed", "ktile_zeroed", "bias_dropped", "edge_shifted")


def feature_rows(n, rows, seed):
    """fp16 [rows, 18, n, n], shaped as extract_agz's rows: plane 2 t = the stones of the player to move t plies ago, 2 t + 1 the
    opponent's, planes 16 / 17 = 1 everywhere if black / white is to move.  Row r is a random order of moves, colours alternating, cut
    after m_r moves: the two colours are disjoint, and with no captures an older plane is a subset of the newer one of its colour.  The
    player to move alternates between rows."""
    rng = np.random.RandomState(seed)
    d = n * n
    out = np.zeros((rows, 18, d), np.float16)
    colour = np.arange(d) & 1                       # move i is black's (0) if i is even
    for r in range(rows):
        order = rng.permutation(d)
        m = rng.randint(d // 4, (3 * d) // 4)
        m += (m ^ r) & 1                            # m & 1 = the colour to move = r & 1
        to_move = m & 1
        for t in range(8):
            cnt = max(m - t, 0)
            cells, col = order[:cnt], colour[:cnt]
            out[r, 2 * t, cells[col == to_move]] = 1
            out[r, 2 * t + 1, cells[col != to_move]] = 1
        out[r, 16 + to_move] = 1
    return torch.from_numpy(out.reshape(rows, 18, n, n))


# ------------------------------------------------------------------------------------------------ roundings

def _h(t):
    """fp64 or fp32 tensor -> the nearest fp16, in ONE rounding (numpy's conversion; a detour over fp32 would round twice)"""
    return torch.from_numpy(t.numpy().astype(np.float16))


def _q(t):
    return _h(t).double()


def _conv_sum(x, w, mode):
    """the sum of a convolution without bias, fp64 in and out: exact (fp64) or, for the proxy, taken in fp32"""
    pad = w.shape[-1] // 2
    if mode == "proxy":
        return Fn.conv2d(x.float(), w.float(), None, 1, pad).double()
    return Fn.conv2d(x, w, None, 1, pad)


def _lin_sum(x, w, mode):
    if mode == "proxy":
        return Fn.linear(x.float(), w.float()).double()
    return Fn.linear(x, w)


def epilogue_of(r1, b, res):
    """the kernels' epilogue behind the rounded sum r1 (fp16): + bias (+ res) in fp32, max(., 0), one rounding to fp16.  b and res hold
    fp16 values."""
    v = r1.float() + b.float()[None, :, None, None]
    if res is not None:
        v = v + res.float()
    return torch.clamp_min(v, 0).half()


def conv_epilogue(acc, b, res):
    """The kernels' two roundings behind the sum `acc` (fp64): fp16; then epilogue_of.  -> (fp16 result, the rounded sum as fp16)"""
    r1 = _h(acc)
    return epilogue_of(r1, b, res), r1


# ------------------------------------------------------------------------------------------------ the net

def build(n, blocks, dim, seed, s, scale=1.0):
    """PolicyValueNet (eval, BatchNorm folded, fp16, on the CPU) whose outputs matter on the rows `s`:
      1. random init; 2. every BatchNorm randomised: gamma = +-U(0.5, 1.5) with 10 % negative, beta and running_mean ~ N(0, 0.3),
      running_var log-uniform in [0.05, 2]; 3. fold_batchnorm; 4. layer by layer in fp64 on `s`, every layer rounded to fp16 before the
      next one is fitted: each trunk convolution's weight and bias rescaled so that its pre-activation (before the skip) has std
      1.0 * scale (input and lower convolutions) or 0.7 * scale (upper), the bias of a block's convolution multiplied by `scale` first
      (without that a dropped bias moves a scale-32 net by less than rounding does: the weights of a convolution between two
      activations of the same scale do not grow, and its bias would stay 1/32 of what it is at scale 1); both head convolutions
      centred through their bias and set to unit std per channel; pi_linear scaled to logits of std 4; value_linear1 to unit std; value_linear2 scaled and centred to a
      pre-tanh of mean 0 and std 1; 5. half()."""
    from elf_amd.net import PolicyValueNet, fold_batchnorm
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = PolicyValueNet(n, 18, blocks, dim).eval()
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                k = m.num_features
                sign = torch.where(torch.rand(k) < 0.1, -1.0, 1.0)
                m.weight.data = sign * (0.5 + torch.rand(k))
                m.bias.data = 0.3 * torch.randn(k)
                m.running_mean.data = 0.3 * torch.randn(k)
                m.running_var.data = torch.exp(torch.empty(k).uniform_(float(np.log(0.05)), float(np.log(2.0))))
    net = fold_batchnorm(net.double())      # in fp64 like everything below: an fp32 fold would differ in its last bit between CPUs
    for p in net.parameters():
        p.requires_grad_(False)

    def fit(mod, x, std, centre=None):
        """rescale mod (Conv2d or Linear) so that mod(x) has the std asked for (and, centred, mean 0: "channel" per output channel,
        "all" over everything); round it to fp16; -> mod(x)"""
        y = mod(x)
        if centre == "channel":
            dims = (0, 2, 3)
            f = std / y.std(dim=dims)
            mean = y.mean(dim=dims)
        else:
            f = (std / y.std()).expand(y.shape[1])
            mean = y.mean().expand(y.shape[1]) if centre == "all" else torch.zeros(y.shape[1], dtype=y.dtype)
        mod.weight.data = _q(mod.weight * f.reshape((-1,) + (1,) * (mod.weight.dim() - 1)))
        mod.bias.data = _q((mod.bias - mean) * f)
        return mod(x)

    with torch.no_grad():
        h = torch.relu(fit(net.init_conv[0], s.double(), 1.0 * scale))
        for b in net.resnet:
            for c in (b.lower[0], b.upper[0]):      # a convolution of activations `scale` times as large: its bias grows with them
                c.bias.data *= scale
            lo = torch.relu(fit(b.lower[0], h, 1.0 * scale))
            h = torch.relu(fit(b.upper[0], lo, 0.7 * scale) + h)
        p = torch.relu(fit(net.pi_final_conv[0], h, 1.0, "channel")).reshape(-1, 2 * net.d)
        fit(net.pi_linear, p, 4.0)
        v = torch.relu(fit(net.value_final_conv[0], h, 1.0, "channel")).reshape(-1, net.d)
        v = torch.relu(fit(net.value_linear1, v, 1.0))
        fit(net.value_linear2, v, 1.0, "all")
    return net.half()


def weights(net):
    """the fp16 parameters of a folded PolicyValueNet as fp64 CPU tensors: convs = [(w [K,C,3,3], b)] of the 1 + 2 * blocks trunk
    convolutions in order, and the five head layers"""
    g = lambda m: (m.weight.detach().cpu().double().contiguous(), m.bias.detach().cpu().double())
    convs = [g(net.init_conv[0])]
    for b in net.resnet:
        convs += [g(b.lower[0]), g(b.upper[0])]
    return dict(convs=convs, pconv=g(net.pi_final_conv[0]), vconv=g(net.value_final_conv[0]), pi=g(net.pi_linear),
                v1=g(net.value_linear1), v2=g(net.value_linear2), d=net.d)


def _mutated_sum(x, w, b, kind):
    """the defects of one convolution: -> (sum, bias)"""
    k, c = w.shape[0], w.shape[1]
    if kind == "tap_zeroed":                        # one tap, for all channels
        w = w.clone()
        w[:, :, 0, 2] = 0
    elif kind == "ktile_zeroed":                    # one 64-channel K tile of one tap (the last tile: all of a 64-channel net's tap)
        w = w.clone()
        w[:, c - 64:, 2, 0] = 0
    elif kind == "bias_dropped":                    # one output channel's bias: the largest one
        b = b.clone()
        b[int(b.abs().argmax())] = 0
    acc = Fn.conv2d(x, w, None, 1, 1)
    if kind == "edge_shifted":                      # the cells of the board's first row read their taps one cell to the left
        xs = torch.zeros_like(x)
        xs[..., 1:] = x[..., :-1]
        acc[:, :, 0, :] = Fn.conv2d(xs, w, None, 1, 1)[:, :, 0, :]
    return acc, b


def forward(W, s, mode="truth", heads="native", mutate=None, first=None):
    """W = weights(net), s = feature rows.  mode "truth" | "emu" | "proxy", heads "native" | "eager" (the module docstring).
    mutate = (kind, block), truth only: a defect in residual block `block`: "skip_dropped", "skip_from_lower" (the skip read from the
    lower convolution's output instead of the block's input), or one of _mutated_sum's in the block's upper convolution.
    first = the fp16 output of the input convolution as a route returned it, taken as given instead of computed: FusedInferenceNet's
    input convolution is MIOpen's, whose sum is not the exact sum rounded once (elf_amd/net.py), so ITS documented sequence starts there.
    -> dict(acts = [fp64 [rows,K,n,n]] after each trunk convolution, logits, pi, pre, V), numpy fp64"""
    assert mode in ("truth", "emu", "proxy") and heads in ("native", "eager") and (mutate is None or mode == "truth")
    rounded = mode != "truth"
    acts = []

    def layer(i, x, res=None, kind=None):
        w, b = W["convs"][i]
        if kind is not None:
            acc, b = _mutated_sum(x, w, b, kind)
        else:
            acc = _conv_sum(x, w, mode)
        if rounded:
            y = conv_epilogue(acc, b, res)[0].double()
        else:
            y = acc + b[None, :, None, None]
            y = torch.relu(y + res if res is not None else y)
        acts.append(y.numpy())
        return y

    with torch.no_grad():
        if first is None:
            h = layer(0, s.double())
        else:
            h = first.detach().cpu().double().contiguous()
            acts.append(h.numpy())
        for blk in range((len(W["convs"]) - 1) // 2):
            kind = mutate[0] if mutate is not None and mutate[1] == blk else None
            assert kind is None or kind in MUTATIONS
            lo = layer(1 + 2 * blk, h)
            res = None if kind == "skip_dropped" else lo if kind == "skip_from_lower" else h
            h = layer(2 + 2 * blk, lo, res, kind if kind not in ("skip_dropped", "skip_from_lower") else None)
        rows, d = h.shape[0], W["d"]
        bc = lambda b: b[None, :, None, None]
        if not rounded or heads == "native":
            # elfnet_heads_f16: fp32 throughout (fp64 for the truth)
            cast = (lambda t: t.float()) if rounded else (lambda t: t)
            x = cast(h)
            p = torch.relu(Fn.conv2d(x, cast(W["pconv"][0])) + bc(cast(W["pconv"][1]))).reshape(rows, 2 * d)
            logits = Fn.linear(p, cast(W["pi"][0]), cast(W["pi"][1]))
            pi = torch.softmax(logits, dim=1)
            v = torch.relu(Fn.conv2d(x, cast(W["vconv"][0])) + bc(cast(W["vconv"][1]))).reshape(rows, d)
            v = torch.relu(Fn.linear(v, cast(W["v1"][0]), cast(W["v1"][1])))
            pre = Fn.linear(v, cast(W["v2"][0]), cast(W["v2"][1])).reshape(rows)
            val = torch.tanh(pre)
        else:
            def conv1(wb):   # Conv2d(1x1) of an fp16 net: the sum -> fp16, + bias -> fp16, ReLU
                c = _h(_conv_sum(h, wb[0], mode))
                return torch.relu((c.float() + bc(wb[1]).float()).half()).double()

            def lin(x, wb):  # Linear of an fp16 net: sum + bias in fp32 -> fp16
                return _h(_lin_sum(x, wb[0], mode) + wb[1]).double()

            logits = lin(conv1(W["pconv"]).reshape(rows, 2 * d), W["pi"])
            pi = torch.softmax(logits.float(), dim=1)
            v = torch.relu(lin(conv1(W["vconv"]).reshape(rows, d), W["v1"]))
            pre = lin(v, W["v2"]).reshape(rows)
            val = torch.tanh(pre.float()).half()
    f64 = lambda t: t.double().numpy()
    return dict(acts=acts, logits=f64(logits), pi=f64(pi), pre=f64(pre), V=f64(val))


# ------------------------------------------------------------------------------------------------ measures

def d(a, b):
    """rms of a - b over all elements"""
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def dmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def conv_nine_taps64(x, w):
    """conv2d(x, w, padding=1) in fp64 on x's device (on the GPU as its nine taps, one fp64 GEMM each): x [rows,C,n,n] (any memory format), w [K,C,3,3] -> [rows,K,n,n]"""
    if not x.is_cuda:       # F.conv2d takes fp64 on the CPU (and is what `forward` sums with); on the GPU MIOpen does not
        return Fn.conv2d(x.double().contiguous(), w.double().contiguous(), None, 1, 1)
    rows, c, hh, ww = x.shape
    xp = Fn.pad(x.double().permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))
    w = w.double()
    out = torch.zeros((rows, hh, ww, w.shape[0]), device=x.device, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + hh, kx:kx + ww, :] @ w[:, :, ky, kx].t()
    return out.permute(0, 3, 1, 2)


def teacher_forced(x, w, b, res, y):
    """One convolution on its own: the fp64 convolution of the fp16 `x` the layer was given, pushed through the kernels' two roundings
    with the `res` it was given, against the fp16 `y` it returned.  Tensors on any device.  -> dict of
      share        the share of elements that differ at all from the two roundings of the fp64 sum
      nan          the number of NaN in y
      outside      THE CRITERION FOR THIS LIBRARY'S KERNELS: the number of elements outside [epilogue(fp16(sum - eps)),
                   epilogue(fp16(sum + eps))].  The epilogue (fp32 additions, max, a rounding) and the rounding of the sum are
                   monotone, so a kernel whose fp32 accumulator is within eps of the exact sum lands inside, whatever its order of
                   summation; for most elements the two ends are one value.  eps is what fp32 accumulation can be off by: a chain
                   of n = 9 C additions whose k-th partial sum is about sqrt(k) t (t the rms of the products) and is rounded by up
                   to 2^-24 of itself, uniformly, has an error of standard deviation 2^-24 t n / sqrt(6) = 2^-24 Q sqrt(n / 6) with
                   Q = sqrt(sum of the squared products), which is computed here per element; the MFMA kernels' 16-term groups
                   and any tree make it smaller.  eps = 6 of these deviations (the test looks at 10^7 elements).  Against the
                   fp16 spacing of a result of size 1 this is 1/250: the interval opens only next to a rounding boundary.
      worst        the first element outside, described
      ulp          the worst error in fp16 ulp, the ulp being the largest of the ulps of the rounded sum, of the expected value and
                   of the result (test_input_conv_real_feature_rows_against_fp64's measure)
      over_one     the number of elements more than one such ulp off.  A correct kernel has some, for two reasons the measure leaves
                   out.  Where fp32(r1 + bias + res) lies exactly between two fp16 values the second rounding is a tie to even, and
                   for a sum one ulp further it is a tie again, decided the other way: two ulp.  And where terms of size 1 cancel
                   to a sum of 1e-5 and bias and skip cancel as well, eps is several ulp of everything in sight.
      bad          THE CRITERION FOR A CONVOLUTION THAT IS NOT THIS LIBRARY'S (MIOpen's input convolution in FusedInferenceNet, whose
                   sum is not an fp32 sum rounded once): the number of elements more than one ulp off that are not bit-equal to the
                   epilogue of an fp16 neighbour of the rounded sum, i.e. not the tie above."""
    acc = conv_nine_taps64(x, w).cpu()
    q = torch.sqrt(conv_nine_taps64(x.double() ** 2, w.double() ** 2)).cpu()
    eps = 6 * 2.0 ** -24 * q * (9 * x.shape[1] / 6) ** 0.5
    b = b.detach().cpu()
    res = None if res is None else res.detach().cpu()
    want, r1 = conv_epilogue(acc, b, res)
    lo, hi = conv_epilogue(acc - eps, b, res)[0].numpy(), conv_epilogue(acc + eps, b, res)[0].numpy()
    near = [epilogue_of(torch.from_numpy(np.nextafter(r1.numpy(), np.float16(to))), b, res).numpy() for to in (np.inf, -np.inf)]
    want, r1, got = want.numpy(), r1.numpy(), y.detach().cpu().numpy()
    ulp = np.maximum(np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got))), np.spacing(np.abs(r1))).astype(np.float32)
    err = np.abs(got.astype(np.float32) - want.astype(np.float32)) / ulp
    nan = int(np.isnan(got).sum())
    over = ~(err <= 1)                  # a NaN is over, and outside
    outside = ~((got >= lo) & (got <= hi))
    bad = over & ~((got == near[0]) | (got == near[1]))
    worst = None
    if outside.any():
        i = tuple(np.argwhere(outside)[0])
        worst = dict(at=tuple(int(v) for v in i), sum64=float(acc.numpy()[i]), eps=float(eps.numpy()[i]), bias=float(b[i[1]]),
                     res=None if res is None else float(res.numpy()[i]), lo=float(lo[i]), hi=float(hi[i]), got=float(got[i]))
    return dict(share=float((got != want).mean()), nan=nan, outside=int(outside.sum()), worst=worst,
                ulp=float(np.nanmax(err)) if nan < got.size else float("nan"), over_one=int(over.sum()), bad=int(bad.sum()))


def decided_rows(T, E, top):
    """rows whose top-`top` set a search may rely on: the gap in T's logits between place `top` and place `top` + 1 is more than
    8 x max |E - T| of the logits (top = 1: the best move against the second).  -> (row indices, T's top sets as sorted arrays)"""
    line = 8 * dmax(E["logits"], T["logits"])
    order = np.argsort(-T["logits"], axis=1)
    srt = np.take_along_axis(T["logits"], order, axis=1)
    ok = np.nonzero(srt[:, top - 1] - srt[:, top] > line)[0]
    return ok, np.sort(order[:, :top], axis=1)


def top_sets(pi_or_logits, top):
    return np.sort(np.argsort(-np.asarray(pi_or_logits, np.float64), axis=1)[:, :top], axis=1)
