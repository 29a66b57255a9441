"""The policy/value net stays on PyTorch-ROCm (BASELINE.json north_star): this module only restates the
ARCHITECTURE of the reference's Model_PolicyValue (src_py/elfgames/go/df_model3.py:113-313: init conv,
num_block residual blocks of two 3x3 conv+BN, 1x1 policy head -> Linear(2*N*N, N*N+1) -> softmax, 1x1 value
head -> Linear(N*N, 256) -> Linear(256, 1) -> tanh) so that benchmarks can run a random-init 20-block/256-channel
net of the right shape and cost.  It is called through the batch interface: forward({"s": ...}) -> {"pi", "V"}.
"""
import torch
import torch.nn as nn


def _conv_bn(cin, cout, k, relu=True):
    layers = [nn.Conv2d(cin, cout, k, padding=k // 2), nn.BatchNorm2d(cout)]
    if relu:
        layers.append(nn.ReLU(inplace=True))
    return nn.Sequential(*layers)


class ResBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.lower = _conv_bn(dim, dim, 3)
        self.upper = _conv_bn(dim, dim, 3, relu=False)

    def forward(self, s):
        return torch.relu(self.upper(self.lower(s)) + s)


class PolicyValueNet(nn.Module):
    def __init__(self, board_size=19, num_planes=18, num_block=20, dim=256):
        super().__init__()
        d = board_size * board_size
        self.d = d
        self.init_conv = _conv_bn(num_planes, dim, 3)
        self.resnet = nn.Sequential(*[ResBlock(dim) for _ in range(num_block)])
        self.pi_final_conv = _conv_bn(dim, 2, 1)
        self.value_final_conv = _conv_bn(dim, 1, 1)
        self.pi_linear = nn.Linear(2 * d, d + 1)
        self.value_linear1 = nn.Linear(d, 256)
        self.value_linear2 = nn.Linear(256, 1)

    def forward(self, batch):
        s = batch["s"] if isinstance(batch, dict) else batch
        p = next(self.parameters())
        s = s.to(dtype=p.dtype)
        if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous():
            s = s.contiguous(memory_format=torch.channels_last)
        s = self.resnet(self.init_conv(s))
        pi = self.pi_linear(self.pi_final_conv(s).reshape(-1, 2 * self.d))
        pi = torch.softmax(pi.float(), dim=1)
        v = torch.relu(self.value_linear1(self.value_final_conv(s).reshape(-1, self.d)))
        v = torch.tanh(self.value_linear2(v)).float().reshape(-1)
        return dict(pi=pi, V=v)


def map_reference_state_dict(sd):
    """Keys of a reference Model_PolicyValue checkpoint (src_py/elfgames/go/df_model3.py:113-313, saved by
    rlpytorch/model_base.py:83-109 as {"state_dict", "step", "options"}) -> keys of PolicyValueNet.  Same tensors, other names:
        [init_conv|pi_final_conv|value_final_conv](.module)?.{0,1}.*   -> unchanged (DataParallel's ".module" dropped)
        resnet(.module)?.resnet.{i}.conv_lower.{0,1}.*                  -> resnet.{i}.lower.{0,1}.*
        resnet(.module)?.resnet.{i}.conv_upper.{0,1}.*                  -> resnet.{i}.upper.{0,1}.*
        pi_linear.* / value_linear1.* / value_linear2.*                 -> unchanged
    Raises KeyError on a key it does not know (nothing is dropped silently)."""
    import re
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) and "state_dict" in sd else sd
    out = {}
    for k, v in sd.items():
        k2 = k.replace(".module.", ".")
        m = re.match(r"^resnet\.resnet\.(\d+)\.conv_(lower|upper)\.(.+)$", k2)
        if m:
            out["resnet.%s.%s.%s" % (m.group(1), m.group(2), m.group(3))] = v
        elif re.match(r"^(init_conv|pi_final_conv|value_final_conv)\.[01]\.", k2) or re.match(r"^(pi_linear|value_linear1|value_linear2)\.", k2):
            out[k2] = v
        else:
            raise KeyError("unknown key in a Model_PolicyValue state_dict: " + k)
    return out


def load_reference_checkpoint(path_or_state, board_size=19, device="cpu"):
    """A PolicyValueNet (eval mode) with the weights of a reference checkpoint (save-*.bin) or of its state_dict.  Block count and
    width are read from the checkpoint itself."""
    sd = torch.load(path_or_state, map_location="cpu") if isinstance(path_or_state, str) else path_or_state
    sd = map_reference_state_dict(sd)
    blocks = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("resnet."))
    dim = sd["init_conv.0.weight"].shape[0]
    planes = sd["init_conv.0.weight"].shape[1]
    net = PolicyValueNet(board_size, planes, blocks, dim)
    net.load_state_dict(sd, strict=True)
    return net.eval().to(device)


def fold_batchnorm(net):
    """Inference-time algebra, not a different net: every Conv2d+BatchNorm2d(eval) pair becomes one Conv2d with
    w' = w * gamma / sqrt(var + eps), b' = (b - mean) * gamma / sqrt(var + eps) + beta (torch.nn.utils.fusion)."""
    from torch.nn.utils.fusion import fuse_conv_bn_eval
    for mod in net.modules():
        if isinstance(mod, nn.Sequential) and len(mod) >= 2 and isinstance(mod[0], nn.Conv2d) and isinstance(mod[1], nn.BatchNorm2d):
            mod[0] = fuse_conv_bn_eval(mod[0], mod[1])
            mod[1] = nn.Identity()
    return net


def chunked_forward(net, s, chunk_rows=2048):
    """net on the rows of `s` in slices of at most chunk_rows (the last one may be shorter): every convolution then has the shape of a
    chunk_rows-row call whatever the number of games in flight -- one MIOpen find (whose verification pass scales with the batch: tens
    of seconds for a 16 384-row shape on a cold database) instead of one per batch size, less activation memory, and the 2048-row
    call is the fastest per position on this part.  -> dict(pi [rows, A] f32, V [rows] f32)"""
    rows = s.shape[0]
    if rows <= chunk_rows:
        return net({"s": s})
    pi = v = None
    for c0 in range(0, rows, chunk_rows):
        o = net({"s": s[c0:c0 + chunk_rows]})
        if pi is None:
            pi = torch.empty((rows, o["pi"].shape[1]), dtype=o["pi"].dtype, device=s.device)
            v = torch.empty((rows,), dtype=o["V"].dtype, device=s.device)
        pi[c0:c0 + chunk_rows].copy_(o["pi"])
        v[c0:c0 + chunk_rows].copy_(o["V"])
    return dict(pi=pi, V=v)


class GraphedNet:
    """The same forward captured once into a HIP graph for a fixed batch shape (PyTorch's CUDAGraph on ROCm): one graph
    launch per batch instead of ~200 eager kernel launches.  forward(batch) copies nothing: `s_static` IS the tensor
    the search writes leaf features into.  Batches above chunk_rows run as slices inside the one graph (chunked_forward)."""

    def __init__(self, net, s_static, chunk_rows=2048):
        self.net, self.s = net, s_static
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(3):
                chunked_forward(net, s_static, chunk_rows)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = chunked_forward(net, s_static, chunk_rows)

    def __call__(self, batch=None):
        self.graph.replay()
        return self.out


def make_net(board_size=19, num_block=20, dim=256, device="cuda", dtype=torch.float16, channels_last=True, seed=0, fold_bn=False):
    """Random-init net (torch.manual_seed(seed)), eval mode, as the benchmark's stand-in for a trained model."""
    torch.manual_seed(seed)
    net = PolicyValueNet(board_size, 18, num_block, dim).eval()
    if fold_bn:
        net = fold_batchnorm(net)
    net = net.to(device=device, dtype=dtype)
    if channels_last:
        net = net.to(memory_format=torch.channels_last)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


class FusedInferenceNet:
    """Inference-only execution of a BN-folded fp16 channels_last PolicyValueNet with bias, skip and ReLU inside the convolutions.

    Eager PyTorch issues conv -> bias add -> ReLU (-> residual add -> ReLU) as separate elementwise kernels, i.e. five HBM round
    trips of the [B,256,N,N] activation per residual block.  Here a 3x3 trunk convolution of an fp16 net is ONE kernel,
    `elfnet_conv3x3_f16`: relu(conv + b) for the lower conv of a block, relu(conv + b + skip) for the upper, and nothing passes over
    the activation a second time.  Behind it are three main loops with one epilogue sequence and the same output bits: algo 1, the
    hand-written 256 x 256 x 64 LDS-DMA kernel (elf_amd/csrc/net_conv3x3.hip), where there are enough positions to fill the chip;
    algo 0, Composable Kernel's implicit GEMM with the tile configuration MIOpen's tuned database picks (elf_amd/csrc/
    net_conv.hip), below that and for the channel counts algo 1 does not take (`_conv_algo`); and, where algo 0 would run, the
    hand-written 64 x 64 x 64 kernel behind `elfnet_conv3x3_small_f16` (elf_amd/csrc/net_conv3x3_small.hip) for calls of at most
    `small_max_positions` positions with C and K multiples of 64: a single game's 16-row call is 364 workgroups there and 46 in
    algo 0 (`_use_small`).
    Every other convolution (the 18-plane input conv, bf16 nets, a weight that is not channels_last) stays a bias-free PyTorch-ROCm
    op (MIOpen) followed by one in-place pass, `elfnet_bias_act_f16` / `_bf16` (elf_amd/csrc/net_epilogue.hip).
    (PyTorch's own fused MIOpen ops, miopen_convolution_relu / miopen_convolution_add_relu, were measured and rejected: for
    fp16 channels_last MIOpen's fusion plan falls back to naive kernels, > 10x slower.)
    Same function as PolicyValueNet.forward (src_py/elfgames/go/df_model3.py:62-110,224-313) up to fp16 rounding: the conv result
    is rounded to fp16 once and the epilogue once, where the eager sequence rounds after every kernel.
    That sequence (the exact sum -> fp16; + bias (+ skip) in fp32, max(., 0); -> fp16) is this library's kernels': on a calibrated
    net every trunk convolution of every route is the documented epilogue of the fp64 sum rounded to fp16 or of an fp16 neighbour of
    it, and differs from the former in 0.01 to 0.02 % of its elements (tests/test_gpu_net_trained_like.py, on an MI355X).  The two
    ends are PyTorch's ops and promise less.  The input convolution is whatever solver MIOpen picks for the shape: measured there, its
    fp16 result is still a neighbour of the rounded exact sum, but another one than it in 13 to 17 % of the elements, so its sum is
    not an fp32 sum rounded once; the final trunk activation is 1.13 to 1.19 times as far from fp64 as the documented sequence's
    (NativeInferenceNet's: 1.00).  And the heads need not return the same bits twice: at 19 x 19 x 256 and 8 rows MIOpen's 1 x 1 policy
    head convolution returned other bits call after call for one activation of that net, in every run of the test (about 1600 of
    5776 outputs; for a random-init net's activation it repeated), which moves pi by up to its distance from fp64 again.
    NativeInferenceNet has neither property.
    Unlike the eager net, a NaN in front of a ReLU becomes 0 (the kernels' max is fmaxf, torch.relu keeps the NaN): a diverged
    activation does not show as NaN in pi or V."""

    # elfnet_conv3x3_f16's algo.  None = by shape (_conv_algo); 0 or 1 pins one.  DESIGN.md section 3 has the probes.
    conv_algo = None
    # algo 1 from this many positions (rows * H * W) on.  The crossover measured on MI355X at 19 x 19 x 256 -> 256, us without /
    # with skip (profiles/conv_pipeline_probe.json): 80 rows, algo 0 55 / 54 against algo 1 53 / 54, inside the spread; 90 rows
    # (32 490 positions) 59 / 57 against 53 / 54, beyond the spread with skip only; 96 rows (34 656 positions) 73 / 73 against
    # 53 / 54.  Algo 1 runs one 36-K-tile workgroup per 256 positions, 53 to 54 us however few there are; algo 0's 256 x 128 tiles
    # are two workgroups per 256 positions and start a second round over the 256 CUs above 128 * 256 positions, which is where it
    # falls behind.
    native_min_positions = 128 * 256 + 1
    # elfnet_conv3x3_small_f16 (64 x 64 x 64 tiles) instead of algo 0 up to this many positions; 0 = never.  Measured on MI355X at
    # 19 x 19 x 256 -> 256, us without / with skip, algo 0 against small (profiles/conv_small_probe.json): 1 row 45.0 / 46.3 against
    # 11.1 / 10.9; 4 rows 45.4 / 46.7 against 11.4 / 11.1; 16 rows (a single game's call) 46.4 / 47.1 against 16.6 / 15.2; 32 rows
    # 49.3 / 52.4 against 25.4 / 25.7; 64 rows (23 104 positions) 55.2 / 56.4 against 48.1 / 48.0, spreads 3.4 / 1.9 and 3.2 / 3.4;
    # 90 rows (32 490) 64.4 / 62.8 against 63.1 / 62.7, inside the spread; 9 x 9: 16 rows 45.3 / 46.6 against 11.3 / 11.1, 404 rows
    # (32 724 positions) 63.3 / 60.1 against 60.9 / 59.8, inside the spread.  So the largest probed size up to which it wins beyond
    # the spread at every probed size below is 64 * 361 = 23 104 (nothing between 64 and 90 rows was probed), and a single game goes
    # from 0.82 to 2.0 moves/s with it (profiles/conv_small_single_game.json).  It ships as 0 all the same: tests/test_gpu_net_edges.py
    # pins an unpinned 9-row call of a 256-channel net to four algo 0 calls of elfnet_conv3x3_f16, which 23 104 would reroute (same
    # bits).  Until that expectation moves the kernel is opt-in: set small_max_positions = 23104 on the class or on an instance.
    small_max_positions = 0

    def __init__(self, net):
        import ctypes as C
        from . import _lib
        p = next(net.parameters())
        if p.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("FusedInferenceNet needs an fp16 or bf16 net")
        self.dtype = p.dtype
        if any(isinstance(m, nn.BatchNorm2d) for m in net.modules()):
            raise ValueError("fold BatchNorm first (make_net(fold_bn=True))")
        self.net, self.C = net, C
        self.L = _lib.lib()   # raises if libelf_amd.so is missing: no silent fallback
        self.check = _lib.check
        conv = lambda seq: seq[0]
        self.first = conv(net.init_conv)
        self.blocks = [(conv(b.lower), conv(b.upper)) for b in net.resnet]

    def _ep(self, x, bias, res, relu=True):
        rows = x.numel() // x.shape[1]
        C = self.C
        fn = self.L.elfnet_bias_act_f16 if self.dtype == torch.float16 else self.L.elfnet_bias_act_bf16
        self.check(fn(C.c_void_p(x.data_ptr()), C.c_void_p(bias.data_ptr()),
                                             C.c_void_p(res.data_ptr()) if res is not None else None, rows, x.shape[1], int(relu),
                                             C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        return x

    def _fusable(self, x, c):
        """The convolutions elfnet_conv3x3_f16 takes: fp16, 3x3, stride 1, pad 1, one group, C and K multiples of 8, and a weight that
        lies in memory as [K,3,3,C] (its strides are checked: a 4-d tensor can claim channels_last without them)."""
        w = c.weight
        k, cin = w.shape[0], w.shape[1]
        return (self.dtype == torch.float16 and tuple(w.shape[2:]) == (3, 3) and tuple(c.stride) == (1, 1)
                and tuple(c.padding) == (1, 1) and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.bias is not None
                and cin % 8 == 0 and k % 8 == 0 and x.shape[1] == cin
                and tuple(w.stride()) == (9 * cin, 1, 3 * cin, cin))

    def _conv_algo(self, positions, cin, k):
        """algo 1 where net_conv3x3.hip takes the shape (C a multiple of 64, K of 256) and measured faster, algo 0 elsewhere"""
        if self.conv_algo is not None:
            return self.conv_algo
        return 1 if cin % 64 == 0 and k % 256 == 0 and positions >= self.native_min_positions else 0

    def _use_small(self, positions, cin, k):
        """net_conv3x3_small.hip instead of algo 0: nothing pinned, a shape it takes (C and K multiples of 64), and few enough
        positions that it measured faster.  Same output bits either way."""
        return (self.conv_algo is None and self._conv_algo(positions, cin, k) == 0 and cin % 64 == 0 and k % 64 == 0
                and positions <= self.small_max_positions)

    def _conv(self, x, c, res=None):
        if not self._fusable(x, c):
            y = torch.nn.functional.conv2d(x, c.weight, None, c.stride, c.padding)
            assert y.is_contiguous(memory_format=torch.channels_last)
            return self._ep(y, c.bias, res)
        assert x.is_contiguous(memory_format=torch.channels_last)
        C = self.C
        n, cin, h, w = x.shape
        k = c.weight.shape[0]
        # a fresh buffer per conv (inside a captured graph it comes from the graph's own pool); x, and res until the upper conv
        # has run, stay alive in the caller
        y = torch.empty((n, k, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        ptrs = (C.c_void_p(x.data_ptr()), C.c_void_p(c.weight.data_ptr()), C.c_void_p(c.bias.data_ptr()),
                C.c_void_p(res.data_ptr()) if res is not None else None, C.c_void_p(y.data_ptr()))
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        if self._use_small(n * h * w, cin, k):
            self.check(self.L.elfnet_conv3x3_small_f16(*ptrs, n, h, w, cin, k, 1, st))
        else:
            self.check(self.L.elfnet_conv3x3_f16(*ptrs, n, h, w, cin, k, 1, self._conv_algo(n * h * w, cin, k), st))
        return y

    @torch.no_grad()
    def __call__(self, batch):
        net = self.net
        s = batch["s"] if isinstance(batch, dict) else batch
        if s.dtype != self.dtype:
            s = s.to(self.dtype)
        s = s.contiguous(memory_format=torch.channels_last)   # no-op for SelfPlay(feature_format="f16_nhwc")
        h = self._conv(s, self.first)
        for lo, up in self.blocks:
            h = self._conv(self._conv(h, lo), up, res=h)
        pi = net.pi_linear(net.pi_final_conv(h).reshape(-1, 2 * net.d))
        pi = torch.softmax(pi.float(), dim=1)
        v = torch.relu(net.value_linear1(net.value_final_conv(h).reshape(-1, net.d)))
        v = torch.tanh(net.value_linear2(v)).float().reshape(-1)
        return dict(pi=pi, V=v)


class NativeInferenceNet(FusedInferenceNet):
    """A BN-folded fp16 channels_last PolicyValueNet from feature rows to pi / V on this library's kernels only:

        elfnet_conv3x3_in_f16  ->  2 x num_block elfnet_conv3x3_f16 or elfnet_conv3x3_small_f16 (FusedInferenceNet's trunk, same `_conv_algo` /
        `_use_small` routing)  ->  elfnet_heads_f16

    No MIOpen convolution, no BLAS GEMM, no PyTorch softmax or tanh inside __call__: no find step on a cold database, no solver
    choice behind the output bits, three launches instead of about fifteen around the trunk.  Same constructor checks and
    {"s"} -> {"pi", "V"} contract as FusedInferenceNet, but fp16 only, and a net any part of which these kernels do not take is
    refused with ValueError: there is no mixed path.
    Same function as FusedInferenceNet up to rounding, with FEWER roundings: the heads run in fp32 from the trunk activation to pi
    and V (elf_amd/csrc/net_io.hip), where the eager ops round to fp16 after the head convolutions and after every Linear.
    A row's pi and V do not depend on the batch it is evaluated in: every kernel sums a row in an order fixed by the shape of one
    row, so one call, chunked_forward and row-by-row calls return the same bits (tests/test_gpu_net_native_io_edges.py, on an MI355X)."""

    def __init__(self, net):
        super().__init__(net)
        if self.dtype != torch.float16:
            raise ValueError("NativeInferenceNet needs an fp16 net")
        from ._lib import ElfNetHeads

        def conv_of(seq, what, ksize, pad):
            c = seq[0]
            if not (isinstance(c, nn.Conv2d) and tuple(c.kernel_size) == (ksize, ksize) and tuple(c.stride) == (1, 1)
                    and tuple(c.padding) == (pad, pad) and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.bias is not None):
                raise ValueError("NativeInferenceNet: %s is not a plain %dx%d convolution with a bias" % (what, ksize, ksize))
            return c

        first = conv_of(net.init_conv, "init_conv", 3, 1)
        k, cin = first.weight.shape[0], first.weight.shape[1]
        if cin % 2 or not 2 <= cin <= 32 or k % 32 or tuple(first.weight.stride()) != (9 * cin, 1, 3 * cin, cin):
            raise ValueError("NativeInferenceNet: elfnet_conv3x3_in_f16 takes an even number of 2 .. 32 input planes, a multiple of "
                             "32 output channels and a channels_last weight")
        dim = k
        for i, b in enumerate(net.resnet):
            for name in ("lower", "upper"):
                c = conv_of(getattr(b, name), "resnet.%d.%s" % (i, name), 3, 1)
                w = c.weight
                if tuple(w.shape[:2]) != (dim, dim) or dim % 8 or tuple(w.stride()) != (9 * dim, 1, 3 * dim, dim):
                    raise ValueError("NativeInferenceNet: resnet.%d.%s is not a channels_last %d -> %d convolution" % (i, name, dim, dim))
        pc, vc = conv_of(net.pi_final_conv, "pi_final_conv", 1, 0), conv_of(net.value_final_conv, "value_final_conv", 1, 0)
        d = net.d
        vh = net.value_linear1.out_features
        shapes = ((pc.weight, (2, dim, 1, 1)), (vc.weight, (1, dim, 1, 1)), (net.pi_linear.weight, (d + 1, 2 * d)),
                  (net.value_linear1.weight, (vh, d)), (net.value_linear2.weight, (1, vh)))
        for w, shape in shapes:
            if tuple(w.shape) != shape:
                raise ValueError("NativeInferenceNet: a head weight of shape %s where %s is expected" % (tuple(w.shape), shape))
        if dim % 8 or any(lin.bias is None for lin in (net.pi_linear, net.value_linear1, net.value_linear2)):
            raise ValueError("NativeInferenceNet: the heads need channels % 8 == 0 and Linear layers with a bias")
        # the tensors elfnet_heads_f16 reads, dense ([2,C,1,1] is [2][C] in memory in either memory format once made contiguous);
        # kept alive here, their addresses in the struct
        flat = lambda t: t.detach().reshape(t.shape[0], -1).contiguous()
        self._head_tensors = [flat(pc.weight), pc.bias.detach().contiguous(), flat(vc.weight), vc.bias.detach().contiguous(),
                              flat(net.pi_linear.weight), net.pi_linear.bias.detach().contiguous(),
                              flat(net.value_linear1.weight), net.value_linear1.bias.detach().contiguous(),
                              flat(net.value_linear2.weight), net.value_linear2.bias.detach().contiguous()]
        if any(t.dtype != torch.float16 or not t.is_cuda for t in self._head_tensors + [first.weight, first.bias]):
            raise ValueError("NativeInferenceNet needs every parameter in fp16 on the GPU")
        self.heads = ElfNetHeads(*[t.data_ptr() for t in self._head_tensors], dim, vh)
        self.dim = dim

    def _conv(self, x, c, res=None):
        if not self._fusable(x, c):   # the constructor has checked the weights: this is a wrong input shape
            raise ValueError("NativeInferenceNet: a convolution elfnet_conv3x3_f16 does not take")
        return super()._conv(x, c, res)

    @torch.no_grad()
    def __call__(self, batch):
        net, C, L = self.net, self.C, self.L
        s = batch["s"] if isinstance(batch, dict) else batch
        if s.dtype != self.dtype:
            s = s.to(self.dtype)
        s = s.contiguous(memory_format=torch.channels_last)   # no-op for SelfPlay(feature_format="f16_nhwc")
        n, cin, hh, ww = s.shape
        if cin != self.first.weight.shape[1] or hh * ww != net.d:
            raise ValueError("NativeInferenceNet: input of shape %s" % (tuple(s.shape),))
        st = C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream)
        h = torch.empty((n, self.dim, hh, ww), dtype=s.dtype, device=s.device, memory_format=torch.channels_last)
        self.check(L.elfnet_conv3x3_in_f16(C.c_void_p(s.data_ptr()), C.c_void_p(self.first.weight.data_ptr()),
                                           C.c_void_p(self.first.bias.data_ptr()), C.c_void_p(h.data_ptr()), n, hh, ww, cin, self.dim, 1, st))
        for lo, up in self.blocks:
            h = self._conv(self._conv(h, lo), up, res=h)
        pi = torch.empty((n, net.d + 1), dtype=torch.float32, device=s.device)
        v = torch.empty((n,), dtype=torch.float32, device=s.device)
        ws_bytes = L.elfnet_heads_workspace(n, hh, ww)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=s.device)
        self.check(L.elfnet_heads_f16(C.c_void_p(h.data_ptr()), C.byref(self.heads), n, hh, ww, C.c_void_p(pi.data_ptr()), net.d + 1,
                                      C.c_void_p(v.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws_bytes, st))
        return dict(pi=pi, V=v)
