"""CPU: which trunk convolutions FusedInferenceNet._use_small (elf_amd/net.py) sends to elfnet_conv3x3_small_f16 instead of algo 0
of elfnet_conv3x3_f16, and that _conv_algo's own answers are what they were.  Nothing here loads libelf_amd.so or touches a GPU."""
import pytest


def _router(small_max=None, conv_algo=None):
    """A FusedInferenceNet with nothing but the attributes the routing reads (its constructor opens libelf_amd.so)"""
    from elf_amd.net import FusedInferenceNet
    f = object.__new__(FusedInferenceNet)
    if small_max is not None:
        f.small_max_positions = small_max
    if conv_algo is not None:
        f.conv_algo = conv_algo
    return f


SHAPES = [(256, 256), (64, 64), (192, 128)]


def test_the_default_is_a_class_attribute_within_the_cap():
    from elf_amd.net import FusedInferenceNet, NativeInferenceNet
    assert isinstance(FusedInferenceNet.small_max_positions, int) and 0 <= FusedInferenceNet.small_max_positions <= 32768
    assert NativeInferenceNet.small_max_positions == FusedInferenceNet.small_max_positions
    assert NativeInferenceNet._use_small is FusedInferenceNet._use_small


@pytest.mark.parametrize("cin,k", SHAPES + [(72, 256), (256, 72)])
def test_off_at_zero(cin, k):
    f = _router(0)
    for positions in (1, 4, 5776, 32768, 32769):
        assert not f._use_small(positions, cin, k)


@pytest.mark.parametrize("limit", [5776, 23104, 32768])
@pytest.mark.parametrize("cin,k", SHAPES)
def test_on_at_and_below_the_threshold_and_off_above(limit, cin, k):
    f = _router(limit)
    for positions in (1, 4, 361, limit - 1, limit):
        assert f._use_small(positions, cin, k), positions
    for positions in (limit + 1, 2 * limit, 2048 * 361):
        assert not f._use_small(positions, cin, k), positions


@pytest.mark.parametrize("cin,k", [(72, 256), (256, 72), (32, 64), (64, 32), (8, 8)])
def test_off_for_channel_counts_the_kernel_refuses(cin, k):
    f = _router(32768)
    for positions in (1, 5776, 32768):
        assert not f._use_small(positions, cin, k)


@pytest.mark.parametrize("pinned", [0, 1])
def test_a_pinned_conv_algo_wins(pinned):
    f = _router(32768, pinned)
    for positions in (1, 5776, 32768, 32769):
        for cin, k in SHAPES + [(72, 256)]:
            assert not f._use_small(positions, cin, k)
            assert f._conv_algo(positions, cin, k) == pinned


def test_off_wherever_conv_algo_says_1():
    """a threshold above native_min_positions does not take calls from algo 1; where algo 1 refuses the channels (K no multiple
    of 256) the call was algo 0's and goes by the threshold alone"""
    f = _router(1 << 30)
    for positions in (32769, 2048 * 361):
        for cin, k in ((256, 256), (64, 256), (192, 512)):
            assert f._conv_algo(positions, cin, k) == 1 and not f._use_small(positions, cin, k)
        for cin, k in ((64, 64), (192, 128)):
            assert f._conv_algo(positions, cin, k) == 0 and f._use_small(positions, cin, k)
    assert f._use_small(32768, 256, 256)


@pytest.mark.parametrize("limit", [None, 0, 5776, 32768, 1 << 30])
def test_conv_algo_answers_are_unchanged(limit):
    from elf_amd.net import FusedInferenceNet
    assert FusedInferenceNet.native_min_positions == 32769 and FusedInferenceNet.conv_algo is None
    f = _router(limit)
    assert f._conv_algo(32768, 256, 256) == 0 and f._conv_algo(32769, 256, 256) == 1
    assert f._conv_algo(1, 256, 256) == 0 and f._conv_algo(2048 * 361, 256, 256) == 1
    assert f._conv_algo(32769, 64, 256) == 1 and f._conv_algo(32769, 192, 512) == 1
    for cin, k in ((64, 64), (256, 128), (72, 256)):
        for positions in (1, 32768, 32769, 2048 * 361, 2 ** 30):
            assert f._conv_algo(positions, cin, k) == 0
