"""GPU: GoGameTrain::act's draws on the device (k_rq_draw, elfrq_dev_*; ReaderQueues.draw_device, ReplayBuffer(device_draws=True))
against the host's elfrq_draw on a second ReaderQueues with the same arguments and inserts -- itself pinned on the reference's
real game thread (test_reader_queues.py, test_gpu_train.py).  Bar: the same int32 triples, call after call."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


class Pair:
    """the host queues and the device-attached ones, given the same inserts"""

    def __init__(self, elf, attach_after=None, **kw):
        self.host, self.dev = elf.ReaderQueues(**kw), elf.ReaderQueues(**kw)
        self.inserted, self.attach_after = 0, attach_after
        if attach_after is None:
            self.dev.attach_device(0)

    def insert(self, slot, num_moves, black_win):
        a, b = self.host.insert(slot, num_moves, black_win), self.dev.insert(slot, num_moves, black_win)
        assert a == b                       # queue index and evicted handle, with and without a handle attached
        self.inserted += 1
        if self.inserted == self.attach_after:
            self.dev.attach_device(0)       # a snapshot of queues that already hold records
        return a

    def check(self, acts, nfa):
        want = np.stack(self.host.draw(acts, nfa))
        got = self.dev.draw_device(acts, nfa).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want)
        assert self.dev.device_status() == 0

    def close(self):
        self.host.close()
        self.dev.close()


def fill(p, count, lengths, black=lambda i: i % 3 == 0, start=0):
    for i in range(start, start + count):
        p.insert(i, lengths(i), black(i))


# T game threads, the acts of consecutive calls: one act; a turn order that starts mid-round with act counts that are no multiple
# of T; threads that draw nothing in a call (and must come back untouched); several 624-word blocks per thread at different phases
@pytest.mark.parametrize("T,calls", [(1, (1, 1)), (3, (7, 5)), (5, (2, 5, 3)), (2, (12, 12))])
@pytest.mark.parametrize("nq,nfa", [(2, 1), (6, 3)])
def test_draws_equal_the_host_call_after_call(elf, T, calls, nq, nfa):
    p = Pair(elf, attach_after=40, num_reader=nq, queue_min_size=2, queue_max_size=50, insert_seed=9, num_threads=T, seed=100 + T)
    fill(p, 120, lambda i: 5 + (i * 7) % 90)
    for acts in calls:
        p.check(acts, nfa)
    p.close()


# nfa = 3.  "half": half the records are 0..2 moves long, so most acts have several lanes that draw again; "rare": one eligible
# record in forty, so every state runs a long chain of tries.  Four acts per thread and more.
@pytest.mark.parametrize("kind,T,acts", [("half", 2, 9), ("rare", 1, 4), ("rare", 3, 13)])
def test_retries_equal_the_host(elf, kind, T, acts):
    p = Pair(elf, num_reader=4, queue_min_size=3, queue_max_size=200, insert_seed=4, num_threads=T, seed=31)
    short = (lambda i: i % 2 == 0) if kind == "half" else (lambda i: i % 40 != 7)
    fill(p, 400, lambda i: i % 3 if short(i) else 3 + i % 60, black=lambda i: (i // 40) % 2 == 0)
    p.check(acts, 3)
    p.check(acts, 3)
    p.close()


# queue_max_size 4 over 4 queues: bursts of inserts and draws in turn until every ring has wrapped many times; bursts shorter and
# longer than the 16 records the rings hold, one longer than an update's chunk of 1024; "black": 9 of 10 games are Black's, so
# even_ratio sits on its clamp.  The last case keeps more positions pending than one chunk, in rings that hold them all.
@pytest.mark.parametrize("qmax,bursts,black", [(4, (16, 3, 5, 1, 21, 9, 1100, 2, 40), "mixed"), (4, (60, 7, 11, 2, 1100, 13), "black"),
                                                 (700, (2500, 1300), "mixed")])
def test_mirror_follows_the_inserts(elf, qmax, bursts, black):
    p = Pair(elf, num_reader=4, queue_min_size=1, queue_max_size=qmax, insert_seed=21, num_threads=2, seed=5)
    is_black = (lambda i: i % 10 != 0) if black == "black" else (lambda i: (i * 5 + i // 7) % 2 == 0)
    at = 0
    for n in bursts:
        fill(p, n, lambda i: 1 + i % 50, black=is_black, start=at)
        at += n
        p.check(3, 1)
    assert all(s == qmax for s in p.host.sizes())     # every ring is full: it has wrapped (many times where it holds 4)
    p.close()


@pytest.mark.parametrize("batchsize,per_launch", [(64, 1), (128, 2)])
def test_replay_buffer_with_device_draws_gives_the_same_batches(elf, batchsize, per_launch):
    import torch
    g = np.load(os.path.join(GOLDEN, "train_act_9.npz"))
    recs = [str(t) for t in g["records"]]
    kw = dict(board_size=9, num_reader=2, queue_min_size=2, queue_max_size=8, batchsize=batchsize, batches_per_launch=per_launch,
              insert_seed=5, seed=12, num_future_actions=3)
    host, dev = elf.ReplayBuffer(**kw), elf.ReplayBuffer(device_draws=True, **kw)

    def same_batches():
        for _ in range(2):
            a, b = host.sample_batches(), dev.sample_batches()
            torch.cuda.synchronize()
            assert len(a) == len(b) == per_launch
            for x, y in zip(a, b):
                for key in x:
                    assert torch.equal(x[key].view(torch.uint8), y[key].view(torch.uint8)), key

    for rb in (host, dev):
        rb.insert(recs[0])
        with pytest.raises(elf.ElfGoError):       # a queue below queue_min_size before the first draw
            rb.sample_batches()
    for t in recs[14:]:
        assert host.insert(t) == dev.insert(t)
    same_batches()
    for t in recs[1:14]:                          # evictions from a full queue, slots reused, records shorter than 3 moves
        assert host.insert(t) == dev.insert(t)
    same_batches()
    q = dev.queues
    assert q.device_status() == 0
    q.attach_device(0)                            # a second call changes nothing
    for bad in (torch.zeros((3, 64), dtype=torch.int64, device=q.device), torch.zeros((3, 63), dtype=torch.int32, device=q.device),
                torch.zeros((3, 64), dtype=torch.int32)):
        with pytest.raises(ValueError):
            q.draw_device(1, 3, out=bad)
    host.close()
    dev.close()
