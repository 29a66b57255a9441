"""CPU: the two pieces of host logic between a batch and the trunk convolution kernels (elf_amd/net.py) -- which algo of
elfnet_conv3x3_f16 FusedInferenceNet._conv_algo routes a call to, and how chunked_forward slices a batch (a short last chunk
included).  Nothing here loads libelf_amd.so or touches a GPU."""
import pytest


def _router(conv_algo=None):
    """A FusedInferenceNet with nothing but the attributes _conv_algo reads (its constructor opens libelf_amd.so)"""
    from elf_amd.net import FusedInferenceNet
    f = object.__new__(FusedInferenceNet)
    if conv_algo is not None:
        f.conv_algo = conv_algo
    return f


def test_conv_algo_threshold_at_256_channels():
    """algo 1 from native_min_positions = 128 * 256 + 1 positions on, algo 0 up to 128 * 256"""
    from elf_amd.net import FusedInferenceNet
    assert FusedInferenceNet.native_min_positions == 32769 and FusedInferenceNet.conv_algo is None
    f = _router()
    assert f._conv_algo(32768, 256, 256) == 0
    assert f._conv_algo(32769, 256, 256) == 1
    assert f._conv_algo(1, 256, 256) == 0
    assert f._conv_algo(2048 * 361, 256, 256) == 1
    # the shapes net_conv3x3.hip takes: C a multiple of 64, K of 256
    assert f._conv_algo(32769, 64, 256) == 1 and f._conv_algo(32769, 192, 512) == 1


@pytest.mark.parametrize("cin,k", [(64, 64), (256, 128), (72, 256)])
@pytest.mark.parametrize("positions", [1, 32768, 32769, 2048 * 361, 2 ** 30])
def test_conv_algo_0_for_the_channel_counts_algo_1_refuses(cin, k, positions):
    assert _router()._conv_algo(positions, cin, k) == 0


@pytest.mark.parametrize("pinned", [0, 1])
def test_a_pinned_conv_algo_wins(pinned):
    f = _router(pinned)
    for positions in (1, 32768, 32769, 2048 * 361):
        for cin, k in ((256, 256), (64, 64), (72, 256)):
            assert f._conv_algo(positions, cin, k) == pinned


class _RowwiseStub:
    """A net whose pi and V of a row depend on that row alone; it keeps the row count of every call"""

    def __init__(self):
        self.seen = []

    def __call__(self, batch):
        import torch
        s = batch["s"]
        self.seen.append(s.shape[0])
        flat = s.reshape(s.shape[0], -1).double()
        pi = torch.stack([flat.sum(1), (flat * flat).sum(1), flat[:, 0] - flat[:, -1]], dim=1).float()
        return dict(pi=pi, V=flat.max(1).values.float())


@pytest.mark.parametrize("chunk_rows,sizes", [(2, [2, 2, 2, 1]), (7, [7]), (8, [7])])
def test_chunked_forward_slices_and_reassembles(chunk_rows, sizes):
    """7 rows in chunks of 2 (a short last chunk), 7 (exactly one) and 8 (one call, below the chunk size): the stub saw those
    chunks in that order, and every row's pi and V are what the stub gives for all rows at once"""
    import torch
    from elf_amd.net import chunked_forward
    # small integers: the stub's sums are exact whatever order a batch size makes torch reduce in
    s = torch.randint(-8, 9, (7, 3, 5, 5), generator=torch.Generator().manual_seed(11)).float()
    want = _RowwiseStub()({"s": s})
    stub = _RowwiseStub()
    out = chunked_forward(stub, s, chunk_rows)
    assert stub.seen == sizes
    assert set(out) == {"pi", "V"}
    assert out["pi"].shape == (7, 3) and out["V"].shape == (7,)
    assert torch.equal(out["pi"], want["pi"]) and torch.equal(out["V"], want["V"])
