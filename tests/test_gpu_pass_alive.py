"""GPU: elfgo_pass_alive (k_pass_alive), GoEngine.pass_alive and GTP elf-pass_alive against Benson's definition restated over sets
of points (pass_alive_expected) and against maps stated by hand.  Every comparison is integer equality."""
import ctypes as C

import numpy as np
import pytest

import pass_alive_expected as PE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def read(eng, k):
    """pass_alive of slots [0, k) -> (map, summary) on the host; the bound-hit flag is 0 in every row"""
    pa = eng.pass_alive(n=k)
    m, s = pa.map.cpu().numpy(), pa.summary.cpu().numpy()
    assert (s[:, [3, 7]] >= 0).all(), "a loop bound was hit"
    for c in (1, 2):
        assert np.array_equal(pa.alive(c).cpu().numpy(), (m >> (c - 1)) & 1 == 1)
        assert np.array_equal(pa.safe(c).cpu().numpy(), (m >> (c + 1)) & 1 == 1)
    return m, s


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("d4", range(8))
def test_constructed_positions(elf, d4, swap):
    n, names = 9, list(PE.POSITIONS)
    want = [PE.constructed(n, name, d4, swap) for name in names]
    eng = elf.GoEngine(n, len(names))
    assert eng.setup(np.array([w[0] for w in want])).cpu().numpy().all()
    m, s = read(eng, len(names))
    for j, (name, (stones, exp, summary)) in enumerate(zip(names, want)):
        assert np.array_equal(m[j], exp), (name, m[j].reshape(n, n).T, exp.reshape(n, n).T)
        assert np.array_equal(s[j], summary), (name, s[j], summary)
        ref = PE.pass_alive(n, stones)
        assert np.array_equal(ref[0], exp) and np.array_equal(ref[1], summary), name
    assert s[names.index("cascade"), 4 * swap + 3] >= 3
    eng.close()


@pytest.mark.parametrize("n,boards,max_steps", [(9, 64, 1 << 20), (9, 64, 40), (19, 16, 1 << 20), (19, 16, 200)])
def test_playout_positions_equal_the_definition(elf, n, boards, max_steps):
    eng = elf.GoEngine(n, boards)
    eng.playout(np.arange(1, boards + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15), max_steps=max_steps)
    col = eng.export_board()[0].cpu().numpy()
    m, s = read(eng, boards)
    want = [PE.pass_alive(n, col[j]) for j in range(boards)]
    wm, ws = np.array([w[0] for w in want]), np.array([w[1] for w in want])
    print("n %d max_steps %d: pass-alive chains black %d white %d, safe points black %d white %d, rounds at most %d" % (
        n, max_steps, ws[:, 0].sum(), ws[:, 4].sum(), ws[:, 2].sum(), ws[:, 6].sum(), ws[:, [3, 7]].max()))
    if max_steps == 1 << 20:   # finished games leave nothing but true eyes: the set holds pass-alive chains of both colours
        assert ws[:, 0].sum() >= 1 and ws[:, 4].sum() >= 1
    bad = np.nonzero((m != wm).any(axis=1) | (s != ws).any(axis=1))[0]
    assert bad.size == 0, (bad.tolist(), s[bad[0]], ws[bad[0]], np.argwhere(m[bad[0]] != wm[bad[0]]).ravel().tolist())
    eng.close()


def test_abi_edges(elf):
    import torch
    from elf_amd._lib import ElfGoError
    n, eng = 9, elf.GoEngine(9, 4)
    stones, exp, summary = PE.constructed(n, "stone_in_eye", 3, 0)
    assert eng.setup(np.array([stones]), ids=[2]).cpu().numpy().all()
    ids = torch.tensor([2, 0, 2], dtype=torch.int32, device=eng.device)
    m = torch.full((3, n * n), 255, dtype=torch.uint8, device=eng.device)
    s = torch.full((3, 8), -7, dtype=torch.int32, device=eng.device)
    call = lambda mp, sp, k=3, idp=ids.data_ptr(): eng.L.elfgo_pass_alive(eng._h, idp, k, mp, sp, eng._stream())
    assert call(C.c_void_p(m.data_ptr()), None) == 0 and call(None, C.c_void_p(s.data_ptr())) == 0
    assert call(None, None) != 0 and call(C.c_void_p(m.data_ptr()), None, k=0) != 0
    assert call(C.c_void_p(m.data_ptr()), None, k=5, idp=None) != 0   # ids NULL over the capacity
    with pytest.raises(ElfGoError):
        eng.pass_alive(n=5)
    m, s = m.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(m[0], exp) and np.array_equal(m[2], exp) and not m[1].any()
    assert np.array_equal(s[0], summary) and np.array_equal(s[2], summary) and s[1].tolist() == [0, 0, 0, 1, 0, 0, 0, 1]
    out = eng.pass_alive(ids=[7, 2])   # a slot id outside the pool
    assert not out.map[0].any() and (out.summary[0] == -1).all() and np.array_equal(out.map[1].cpu().numpy(), exp)
    eng.close()


def test_gtp(elf):
    import torch
    from elf_amd.gtp import GtpEngine
    n = 9
    actor = lambda batch: dict(pi=torch.full((batch["s"].shape[0], n * n + 1), 1.0 / (n * n + 1), device="cuda"),
                               V=torch.zeros(batch["s"].shape[0], device="cuda"))
    eng = GtpEngine(actor, board_size=n, mcts_rollout_per_thread=16, nodes_per_game=1024)
    assert "elf-pass_alive" in eng.command("list_commands").split() and eng.command("known_command elf-pass_alive") == "= true\n\n"
    assert eng.command("elf-pass_alive") == "= \n\n" == eng.command("elf-pass_alive territory")
    eng.sp.setup(PE.constructed(n, "two_eyes", 0, 0)[0], [0], 1)
    # two_eyes: stones (1,0) (3,0) and (0..3,1), eyes (0,0) and (2,0); board order is x-major, the vertex of (x, y) is letter x, y + 1
    assert eng.command("elf-pass_alive") == "= A2 B1 B2 C2 D1 D2\n\n"
    assert eng.command("elf-pass_alive territory") == "= A1 C1\n\n"
    assert eng.command("elf-pass_alive stones").startswith("?")
    eng.close()
