"""Host side of the board engine: a thin, batch-oriented mirror of the reference's GoState /
BoardFeature interface over the C ABI (include/elf_amd.h).

Reference interface mirrored (src_cpp/elfgames/go/base/):
  GoState::reset / copy-ctor / forward / checkMove / terminated / evaluate   go_state.{h,cc}
  BoardFeature::extractAGZ / coord2Action / action2Coord / setD4Code         board_feature.{h,cc}
Every call works on a batch of board slots that live in HBM; torch is used only to own device
buffers and streams.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check

M_PASS, M_RESIGN, M_SKIP, M_INVALID, M_CLEAR = 0, 1, 2, 3, 4  # base/common.h:43-47
S_EMPTY, S_BLACK, S_WHITE, S_OFF_BOARD = 0, 1, 2, 3           # base/common.h:36-39
NUM_AGZ_PLANES = 18                                           # base/board_feature.h:38
NUM_DF_PLANES = 25                                            # base/board_feature.h:18
INFO_WORDS = 16
INFO_FIELDS = ("ply", "next_player", "last_move", "last_move2", "ko_age", "simple_ko", "simple_ko_color",
               "b_cap", "w_cap", "terminated", "superko", "hist_len", "sk_len", "hash_lo", "hash_hi")


def coord(n, x, y):
    """OFFSETXY (base/board.h:183-184)"""
    return (y + 1) * (n + 2) + (x + 1)


def coord_xy(n, c):
    """X(c), Y(c) (base/board.h:178-179)"""
    return c % (n + 2) - 1, c // (n + 2) - 1


def d4_transform(n, d4, x, y):
    """BoardFeature::Transform (base/board_feature.h:97-113)"""
    rot, flip = d4 % 4, (d4 >> 2) == 1
    if rot == 1:
        x, y = y, n - x - 1
    elif rot == 2:
        x, y = n - x - 1, n - y - 1
    elif rot == 3:
        x, y = n - y - 1, x
    if flip:
        x, y = y, x
    return x, y


def d4_inv_transform(n, d4, x, y):
    """BoardFeature::InvTransform (base/board_feature.h:115-130)"""
    rot, flip = d4 % 4, (d4 >> 2) == 1
    if flip:
        x, y = y, x
    if rot == 1:
        x, y = n - y - 1, x
    elif rot == 2:
        x, y = n - x - 1, n - y - 1
    elif rot == 3:
        x, y = y, n - x - 1
    return x, y


def coord2action(n, d4, c):
    """BoardFeature::coord2Action (base/board_feature.h:132-137)"""
    if c == M_PASS:
        return n * n
    x, y = d4_transform(n, d4, *coord_xy(n, c))
    return x * n + y


def action2coord(n, d4, a):
    """BoardFeature::action2Coord (base/board_feature.h:139-144)"""
    if a == -1 or a == n * n:
        return M_PASS
    x, y = d4_inv_transform(n, d4, a // n, a % n)
    return coord(n, x, y)


SUMMARY_FIELDS = ("score_chinese", "score_japanese", "black_lives", "white_lives", "left", "top", "right", "bottom", "attacker",
                  "living_black", "living_white", "reserved")
EYE, FAKE_EYE, TRUE_EYE, SEMI_EYE = 1, 2, 4, 8   # Black's bits of LifeMap.eye; White's are these << 4


class LifeMap:
    """What GoEngine.life_map returns: the device tensors of elfgo_life_map, and getEyeColor derived from them."""

    def __init__(self, eye, semi_move, alive, summary):
        self.eye, self.semi_move, self.alive, self.summary = eye, semi_move, alive, summary

    @property
    def eye_colour(self):
        """getEyeColor (base/board.cc:1916-1922) per point: 2 where it is White's true eye (asked first), 1 where Black's, else 0"""
        white, black = (self.eye & (TRUE_EYE << 4)) != 0, (self.eye & TRUE_EYE) != 0
        return white.to(torch.uint8) * 2 + (black & ~white).to(torch.uint8)


LD_INFO_FIELDS = ("left", "top", "right", "bottom", "attacker", "defender", "to_move", "lives")
LD_STAT_FIELDS = ("lived", "survived", "defender_stones", "attacker_stones", "superko", "steps", "hash_sum", "reserved")


class LdReading:
    """What GoEngine.ld_read returns: the device tensors of elfgo_ld_run -- info int32 [k, 8] (LD_INFO_FIELDS), stats int64 [k, 8]
    (LD_STAT_FIELDS), first int32 [k, 3, N*N + 1] (per first move, index N*N = pass: playouts, lived, survived) -- and what is
    derived from them."""

    def __init__(self, n, playouts, info, stats, first):
        self.n, self.playouts, self.info, self.stats, self.first = n, playouts, info, stats, first

    @property
    def live_rate(self):
        """playouts at whose end OneGroupLives(defender, box) holds / playouts -> float64 [k]"""
        return self.stats[:, 0].to(torch.float64) / self.playouts

    @property
    def survive_rate(self):
        """playouts at whose end the defender has a stone inside the box / playouts -> float64 [k]"""
        return self.stats[:, 1].to(torch.float64) / self.playouts

    def best_move(self):
        """Per row the first move to play -> list of actions (a = x*N + y; N*N = pass; None where no playout made a move).  Among
        the first moves with at least one playout: the largest lived / playouts when the side to move is the defender, the
        smallest when it is the attacker; ratios are compared by integer cross-multiplication; ties go to the move with more
        playouts, then to the smaller action."""
        first = self.first.cpu().numpy().astype(np.int64)
        info = self.info.cpu().numpy()
        out = []
        for i in range(first.shape[0]):
            sign = 1 if info[i, 6] == info[i, 5] else -1
            best = None
            for a in np.nonzero(first[i, 0])[0]:
                p, l = int(first[i, 0, a]), int(first[i, 1, a])
                if best is None:
                    best = (int(a), p, l)
                    continue
                _, bp, bl = best
                d = sign * (l * bp - bl * p)       # > 0: a's ratio is the better one
                if d > 0 or (d == 0 and p > bp):   # actions come in ascending order: a tie on both keeps the smaller
                    best = (int(a), p, l)
            out.append(None if best is None else best[0])
        return out


class GoEngine:
    """A pool of `capacity` boards of one size resident in HBM on `device`.
    track_placed=True keeps, beside the slots, the ply at which every stone was placed (an ElfGoDf handle, include/elf_amd.h):
    reset / copy / setup / forward go through the elfgo_df_* forms, extract_df() and placed() work, and playout() -- which
    plays on the slots without the table -- raises."""

    def __init__(self, board_size=19, capacity=4096, device=0, track_placed=False):
        if not torch.cuda.is_available():
            raise RuntimeError("elf_amd.GoEngine needs a ROCm GPU (no CPU fallback exists)")
        self.L = _lib.lib()
        self.n = int(board_size)
        self.capacity = int(capacity)
        self.device = torch.device("cuda", device)
        self.num_action = self.n * self.n + 1
        z = np.fromfile(_lib.ZOBRIST_BIN, dtype="<u8")
        if z.size != 441:
            raise RuntimeError("bad zobrist table")
        zz = np.ascontiguousarray(z[: (self.n + 2) ** 2])
        h = C.c_void_p()
        check(self.L.elfgo_create(self.n, self.capacity, device, zz.ctypes.data, C.byref(h)))
        self._h = h
        self._df = None
        if track_placed:
            d = C.c_void_p()
            check(self.L.elfgo_df_create(self._h, C.byref(d)))
            self._df = d

    @classmethod
    def borrow(cls, handle, board_size, capacity, device):
        """A non-owning view of an engine another object owns (the game boards of a SelfPlay): close() does not destroy it."""
        self = cls.__new__(cls)
        self.L = _lib.lib()
        self.n, self.capacity, self.device = int(board_size), int(capacity), device
        self.num_action = self.n * self.n + 1
        self._h = C.c_void_p(handle)
        self._borrowed = True
        self._df = None   # whoever owns the engine plays on it without a table
        return self

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_own", None):
                self.L.elfgo_own_destroy(self._own[1])
                self._own = None
            if getattr(self, "_df", None):
                self.L.elfgo_df_destroy(self._df)
                self._df = None
            if not getattr(self, "_borrowed", False):
                self.L.elfgo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _ids(self, ids, n=None):
        """-> (device int32 tensor or None, pointer, count)"""
        if ids is None:
            k = self.capacity if n is None else n
            return None, None, k
        t = torch.as_tensor(ids, dtype=torch.int32, device=self.device).contiguous()
        return t, C.c_void_p(t.data_ptr()), t.numel()

    def _i32(self, v, n):
        if v is None:
            return None, None
        t = torch.as_tensor(v, dtype=torch.int32, device=self.device).contiguous()
        assert t.numel() == n
        return t, C.c_void_p(t.data_ptr())

    def _boxes(self, regions, k, device_ok=False):
        """k host boxes (left, top, right, bottom) -> device int32 [k, 4], or None for None; a box outside 0 <= left <= right <= N,
        0 <= top <= bottom <= N raises ValueError.  device_ok (region_moves, ld_read): a device int32 tensor [k, 4] is used as it
        is, unread by the host: the kernels clamp each value into [0, N], and a box with left > right or top > bottom is empty."""
        if regions is None:
            return None
        if device_ok and isinstance(regions, torch.Tensor) and regions.is_cuda:
            if regions.dtype != torch.int32 or tuple(regions.shape) != (k, 4):
                raise ValueError("a device regions tensor must be int32 [%d, 4]" % k)
            return regions.contiguous()
        r = np.asarray(regions, dtype=np.int64).reshape(-1, 4)
        if r.shape[0] != k:
            raise ValueError("regions must hold one box per row (%d), got %d" % (k, r.shape[0]))
        ok = (0 <= r[:, 0]) & (r[:, 0] <= r[:, 2]) & (r[:, 2] <= self.n) & (0 <= r[:, 1]) & (r[:, 1] <= r[:, 3]) & (r[:, 3] <= self.n)
        if not ok.all():
            raise ValueError("box %s of row %d is not inside 0 <= left <= right <= N, 0 <= top <= bottom <= N"
                             % (tuple(int(v) for v in r[int(np.nonzero(~ok)[0][0])]), int(np.nonzero(~ok)[0][0])))
        return torch.from_numpy(np.ascontiguousarray(r, dtype=np.int32)).to(self.device)

    def sync(self):
        check(self.L.elfgo_sync(self._h, self._stream()))

    # ---- GoState surface (batched)
    def reset(self, ids=None):
        t, p, k = self._ids(ids)
        if self._df:
            check(self.L.elfgo_df_reset(self._df, p, k, self._stream()))
        else:
            check(self.L.elfgo_reset(self._h, p, k, self._stream()))

    def copy(self, dst_ids, src_ids):
        d, dp, k = self._ids(dst_ids)
        s, sp, k2 = self._ids(src_ids)
        assert k == k2
        if self._df:
            check(self.L.elfgo_df_copy(self._df, dp, sp, k, self._stream()))
        else:
            check(self.L.elfgo_copy(self._h, dp, sp, k, self._stream()))

    def setup(self, stones, ids=None, next_player=None):
        """Put stones on boards (elfgo_setup): stones [k, N*N] or [N*N] uint8 (0 empty, 1 black, 2 white, index a = x*N + y --
        what export_board()[0] returns, so `eng.setup(eng.export_board(src)[0], dst)` copies positions without their
        history), next_player per row (1 / 2; None = Black).  Returns uint8 tensor: 1 set up, 0 refused (a byte above 2, a
        player other than 1 / 2, a group without a liberty); a refused slot is left as it was."""
        st = torch.as_tensor(stones, dtype=torch.uint8, device=self.device).reshape(-1, self.n * self.n).contiguous()
        k = st.shape[0]
        t, p, k2 = self._ids(ids, k)
        assert k2 == k
        npl = None
        if next_player is not None:
            npl = torch.as_tensor(next_player, dtype=torch.uint8, device=self.device).reshape(-1).contiguous()
            if npl.numel() == 1 and k > 1:
                npl = npl.repeat(k)
            assert npl.numel() == k
        ok = torch.empty(k, dtype=torch.uint8, device=self.device)
        fn, h = (self.L.elfgo_df_setup, self._df) if self._df else (self.L.elfgo_setup, self._h)
        check(fn(h, p, C.c_void_p(st.data_ptr()), C.c_void_p(npl.data_ptr()) if npl is not None else None, k,
                 C.c_void_p(ok.data_ptr()), self._stream()))
        return ok

    def forward(self, ids, moves):
        """GoState::forward for each (slot, Coord). Returns uint8 tensor: 1 played, 0 refused, 255 M_INVALID."""
        mv = torch.as_tensor(moves, dtype=torch.int32, device=self.device).contiguous()
        t, p, k = self._ids(ids, mv.numel())
        assert k == mv.numel()
        ok = torch.empty(k, dtype=torch.uint8, device=self.device)
        fn, h = (self.L.elfgo_df_forward, self._df) if self._df else (self.L.elfgo_forward, self._h)
        check(fn(h, p, C.c_void_p(mv.data_ptr()), k, C.c_void_p(ok.data_ptr()), self._stream()))
        return ok

    def legal_mask(self, ids=None, n=None):
        t, p, k = self._ids(ids, n)
        out = torch.empty((k, self.num_action), dtype=torch.uint8, device=self.device)
        check(self.L.elfgo_legal_mask(self._h, p, k, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def extract_agz(self, ids=None, d4=None, out=None, n=None, fmt="f32_nchw"):
        """BoardFeature::extractAGZ into `out` [k,18,N,N] (allocated if None): the batcher's "s" tensor.
        fmt "f32_nchw": fp32 contiguous rows (the reference's layout); "f16_nhwc": fp16 channels_last rows, i.e. what
        an fp16 channels_last net reads without a cast/permute pass."""
        t, p, k = self._ids(ids, n)
        d, dp = self._i32(d4, k)
        f16 = fmt == "f16_nhwc"
        if not f16 and fmt != "f32_nchw":
            raise ValueError("fmt must be 'f32_nchw' or 'f16_nhwc'")
        row = NUM_AGZ_PLANES * self.n * self.n
        if out is None:
            if f16:
                out = torch.empty((k, self.n, self.n, NUM_AGZ_PLANES), dtype=torch.float16, device=self.device).permute(0, 3, 1, 2)
            else:
                out = torch.empty((k, NUM_AGZ_PLANES, self.n, self.n), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.shape[0] >= k and out.dtype == (torch.float16 if f16 else torch.float32)
        inner = (1, self.n * NUM_AGZ_PLANES, NUM_AGZ_PLANES) if f16 else (self.n * self.n, self.n, 1)
        assert tuple(out.stride()[1:]) == inner, "rows must be %s" % ("channels_last" if f16 else "contiguous [18,N,N]")
        stride = out.stride(0) if out.shape[0] > 1 else row
        check(self.L.elfgo_extract_agz_fmt(self._h, p, dp, k, C.c_void_p(out.data_ptr()), stride, 1 if f16 else 0, self._stream()))
        return out

    def extract_df(self, ids=None, d4=None, out=None, n=None):
        """BoardFeature::extract, the reference's 25 DarkForest planes (liberty classes, simple ko, stones, exponential move
        history, distance maps, colour indicators; include/elf_amd.h lists them), into `out` [k,25,N,N] float32 (allocated if
        None; rows contiguous [25,N,N], any row stride).  A row whose slot id lies outside the pool is all zero.  Needs
        track_placed=True: the history planes read the ply at which each stone was placed."""
        if not self._df:
            raise ValueError("extract_df needs GoEngine(..., track_placed=True)")
        t, p, k = self._ids(ids, n)
        d, dp = self._i32(d4, k)
        row = NUM_DF_PLANES * self.n * self.n
        if out is None:
            out = torch.empty((k, NUM_DF_PLANES, self.n, self.n), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.shape[0] >= k and out.dtype == torch.float32
        assert tuple(out.stride()[1:]) == (self.n * self.n, self.n, 1), "rows must be contiguous [25,N,N]"
        stride = out.stride(0) if out.shape[0] > 1 else row
        check(self.L.elfgo_df_extract(self._df, p, dp, k, C.c_void_p(out.data_ptr()), stride, self._stream()))
        return out

    def placed(self, ids=None, n=None):
        """-> int16 tensor [k, N*N], index a = x*N + y: the ply at which the stone on the point was placed (Info::last_placed);
        entries of empty points are stale or 0.  Needs track_placed=True."""
        if not self._df:
            raise ValueError("placed needs GoEngine(..., track_placed=True)")
        t, p, k = self._ids(ids, n)
        out = torch.empty((k, self.n * self.n), dtype=torch.int16, device=self.device)
        check(self.L.elfgo_df_placed(self._df, p, k, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def evaluate(self, ids=None, komi=7.5, n=None):
        t, p, k = self._ids(ids, n)
        out = torch.empty(k, dtype=torch.float32, device=self.device)
        check(self.L.elfgo_evaluate(self._h, p, k, float(komi), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def info(self, ids=None, n=None):
        """-> int32 tensor [k,16] on device; see INFO_FIELDS"""
        t, p, k = self._ids(ids, n)
        out = torch.empty((k, INFO_WORDS), dtype=torch.int32, device=self.device)
        check(self.L.elfgo_info(self._h, p, k, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def info_host(self, ids=None, n=None):
        a = self.info(ids, n).cpu().numpy()
        d = {f: a[:, i].copy() for i, f in enumerate(INFO_FIELDS)}
        d["hash"] = (a[:, 13].astype(np.uint32).astype(np.uint64)) | (a[:, 14].astype(np.uint32).astype(np.uint64) << np.uint64(32))
        return d

    def export_board(self, ids=None, n=None):
        t, p, k = self._ids(ids, n)
        col = torch.empty((k, self.n * self.n), dtype=torch.uint8, device=self.device)
        lib = torch.empty((k, self.n * self.n), dtype=torch.int16, device=self.device)
        check(self.L.elfgo_export_board(self._h, p, k, C.c_void_p(col.data_ptr()), C.c_void_p(lib.data_ptr()), self._stream()))
        return col, lib

    def _seeds(self, seeds, ids):
        """One uint64 seed per listed slot (numpy or int64-viewed tensor) -> (device tensor, ids tensor, ids pointer, rows)."""
        if isinstance(seeds, torch.Tensor):
            sd = seeds.to(self.device).contiguous()
        else:
            sd = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint64).view(np.int64)).to(self.device)
        k = sd.numel()
        t, p, k2 = self._ids(ids, k)
        assert k2 == k
        return sd, t, p, k

    def playout(self, seeds, ids=None, max_steps=1 << 20, out=None, self_atari_thres=None):
        """config-2 protocol: random legal non-true-eye play to game end, whole games in one launch.
        seeds: uint64 per board (numpy or int64-viewed tensor). Returns uint32-as-int64 tensor [k,4] =
        hash_lo, hash_hi, ply, steps.
        self_atari_thres=t plays from the reference's FindAllCandidateMoves(board, player, t) instead (elfgo_playout_cand): the
        same list minus the self-ataris of t stones or more; None is elfgo_playout itself."""
        if self._df:
            raise ValueError("playout plays on the slots without the placement table: not on a track_placed engine")
        sd, t, p, k = self._seeds(seeds, ids)
        if out is None:
            out = torch.empty((k, 4), dtype=torch.int32, device=self.device)
        if self_atari_thres is None:
            check(self.L.elfgo_playout(self._h, p, C.c_void_p(sd.data_ptr()), k, int(max_steps), C.c_void_p(out.data_ptr()), self._stream()))
        else:
            check(self.L.elfgo_playout_cand(self._h, p, C.c_void_p(sd.data_ptr()), k, int(max_steps), int(self_atari_thres),
                                            C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # ---- per-point answers
    def area_map(self, ids=None, n=None):
        """Tromp-Taylor area per point -> uint8 tensor [k, N*N]: 0 neutral, 1 black, 2 white, index a = x*N + y."""
        t, p, k = self._ids(ids, n)
        out = torch.empty((k, self.n * self.n), dtype=torch.uint8, device=self.device)
        check(self.L.elfgo_area_map(self._h, p, k, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def ladder_map(self, ids=None, n=None, with_calls=False):
        """Ladder reading for the side to move (checkLadder, base/board.cc:476-524) -> int16 tensor [k, N*N], index a = x*N + y:
        d > 0 where the mover would extend a group out of atari and still be captured in a ladder after d plies, else 0.
        with_calls=True returns (depth, calls): calls is the reference's num_call of each point's search, 0 where none ran,
        -1 where a bound of the device search cut it (that point's depth is 0)."""
        t, p, k = self._ids(ids, n)
        depth = torch.empty((k, self.n * self.n), dtype=torch.int16, device=self.device)
        calls = torch.empty((k, self.n * self.n), dtype=torch.int16, device=self.device) if with_calls else None
        check(self.L.elfgo_ladder_map(self._h, p, k, C.c_void_p(depth.data_ptr()), C.c_void_p(calls.data_ptr()) if with_calls else None,
                                      self._stream()))
        return (depth, calls) if with_calls else depth

    def candidates(self, ids=None, n=None, self_atari_thres=1):
        """Self-atari reading for the side to move (isSelfAtari, base/board.cc:254-297, and FindAllCandidateMoves, :850-890)
        -> (mask uint8 [k, N*N], stones int16 [k, N*N]), index a = x*N + y: mask is 1 on the legal points that are neither
        the mover's own true eye nor a self-atari of self_atari_thres stones or more; stones is the size of the group a move
        there would leave with exactly one liberty, 0 where it is no self-atari (or illegal).  A row whose slot id lies
        outside the pool gets mask 0 and stones -1."""
        t, p, k = self._ids(ids, n)
        mask = torch.empty((k, self.n * self.n), dtype=torch.uint8, device=self.device)
        stones = torch.empty((k, self.n * self.n), dtype=torch.int16, device=self.device)
        check(self.L.elfgo_candidates(self._h, p, k, int(self_atari_thres), C.c_void_p(mask.data_ptr()), C.c_void_p(stones.data_ptr()),
                                      self._stream()))
        return mask, stones

    def life_map(self, ids=None, n=None, regions=None):
        """The reference's static life reading of each position, both colours at once (elfgo_life_map) -> LifeMap with device
        tensors, index a = x*N + y:
          eye uint8 [k, N*N]: Black's answers in bits 0-3, White's in bits 4-7: bit 0 isEye, 1 isFakeEye, 2 isTrueEye, 3 isSemiEye
            (base/board.cc:1850-1914); isFakeEye is answered at every point, the others are 0 off empty points;
          semi_move int16 [k, 2, N*N]: the action isSemiEye names where it holds for Black / White, else -1;
          alive uint8 [k, N*N]: 1 on the stones of groups that live by two eyes (GivenGroupLives, board.cc:1108-1181);
          summary int32 [k, 12]: see SUMMARY_FIELDS (getFastScore under both rules, OneGroupLives per colour over the box, the
            box, GuessLDAttacker, living groups per colour in the box);
          eye_colour uint8 [k, N*N]: getEyeColor (0 / 1 / 2), derived from eye.
        regions: a host sequence of k boxes (left, top, right, bottom), half-open in x and y as the reference's Region; None =
        getBoardBBox of each row.  A box outside 0 <= left <= right <= N, 0 <= top <= bottom <= N raises ValueError before
        anything is launched.  A row whose slot id lies outside the pool gets maps 0, semi_move -1 and summary -1."""
        t, p, k = self._ids(ids, n)
        reg = self._boxes(regions, k)
        np_ = self.n * self.n
        eye = torch.empty((k, np_), dtype=torch.uint8, device=self.device)
        semi = torch.empty((k, 2, np_), dtype=torch.int16, device=self.device)
        alive = torch.empty((k, np_), dtype=torch.uint8, device=self.device)
        summary = torch.empty((k, len(SUMMARY_FIELDS)), dtype=torch.int32, device=self.device)
        check(self.L.elfgo_life_map(self._h, p, k, C.c_void_p(reg.data_ptr()) if reg is not None else None, C.c_void_p(eye.data_ptr()),
                                    C.c_void_p(semi.data_ptr()), C.c_void_p(alive.data_ptr()), C.c_void_p(summary.data_ptr()),
                                    self._stream()))
        return LifeMap(eye, semi, alive, summary)

    def fast_score(self, ids=None, n=None, rule="chinese"):
        """getFastScore (base/board.cc:1924-1952) from Black's side -> int32 tensor [k]: stones plus true eyes under "chinese",
        true eyes plus captures under "japanese"; no komi, as in the reference."""
        if rule not in ("chinese", "japanese"):
            raise ValueError("rule must be 'chinese' or 'japanese'")
        t, p, k = self._ids(ids, n)
        summary = torch.empty((k, len(SUMMARY_FIELDS)), dtype=torch.int32, device=self.device)
        check(self.L.elfgo_life_map(self._h, p, k, None, None, None, None, C.c_void_p(summary.data_ptr()), self._stream()))
        return summary[:, 0 if rule == "chinese" else 1].contiguous()

    def _own_handle(self, max_lanes):
        """the ElfGoOwnership scratch handle for `max_lanes`, made on first use and remade when max_lanes changes -> (max_lanes, handle)"""
        own = getattr(self, "_own", None)
        if own is None or own[0] != int(max_lanes):
            if own is not None:
                self.sync()
                self.L.elfgo_own_destroy(own[1])
                self._own = None
            h = C.c_void_p()
            check(self.L.elfgo_own_create(self._h, int(max_lanes), C.byref(h)))
            self._own = own = (int(max_lanes), h)
        return own

    def ownership(self, seeds, ids=None, playouts=256, komi=7.5, max_steps=1 << 20, max_lanes=0, self_atari_thres=None):
        """Monte-Carlo ownership: `playouts` config-2 playouts from a private copy of each listed slot (the slots themselves are
        only read), playout k of row i with seed seeds[i] + k * 0x9E3779B97F4A7C15 (mod 2^64).  Returns a dict:
        counts int32 [k, 2, N*N] (playouts in which the point ended as black / white area) and stats int64 [k, 4] (sum of
        black - white area, black wins after komi, super-ko endings, steps played) straight from the device, and derived from
        them own = (black - white) / playouts float32 [k, N*N], score_mean = mean area difference - komi, black_win_rate.
        The scratch handle is made on first use and lives until close(); max_lanes bounds the playouts in flight (0 = a default
        from the CU count).  A row whose slot id lies outside the pool is not played: its counts and stats are zero, as in
        ld_read.  self_atari_thres=t plays the candidate policy of playout(self_atari_thres=t)
        (elfgo_own_run_cand); None is elfgo_own_run itself."""
        sd, t, p, k = self._seeds(seeds, ids)
        own = self._own_handle(max_lanes)
        counts = torch.empty((k, 2, self.n * self.n), dtype=torch.int32, device=self.device)
        stats = torch.empty((k, 4), dtype=torch.int64, device=self.device)
        if self_atari_thres is None:
            check(self.L.elfgo_own_run(own[1], p, C.c_void_p(sd.data_ptr()), k, int(playouts), int(max_steps), float(komi),
                                       C.c_void_p(counts.data_ptr()), C.c_void_p(stats.data_ptr()), self._stream()))
        else:
            check(self.L.elfgo_own_run_cand(own[1], p, C.c_void_p(sd.data_ptr()), k, int(playouts), int(max_steps), float(komi),
                                            int(self_atari_thres), C.c_void_p(counts.data_ptr()), C.c_void_p(stats.data_ptr()),
                                            self._stream()))
        return dict(counts=counts, stats=stats,
                    own=(counts[:, 0] - counts[:, 1]).to(torch.float32) / playouts,
                    score_mean=stats[:, 0].to(torch.float64) / playouts - komi,
                    black_win_rate=stats[:, 1].to(torch.float64) / playouts)

    def region_moves(self, ids=None, n=None, regions=None, self_atari_thres=1):
        """The reference's Region lists for the side to move (elfgo_region_moves) -> (cand, valid, groups), uint8 [k, N*N], index
        a = x*N + y: cand is FindAllCandidateMovesInRegion(board, box, next_player, self_atari_thres) (candidates()'s mask clipped
        to the box), valid is FindAllValidMovesInRegion (the legal points inside the box), groups is 1 on every stone of a group
        that has a stone inside the box (GroupInRegion).  regions: a host sequence of k boxes (left, top, right, bottom),
        half-open, validated as life_map validates them (ValueError before anything is launched), or a device int32 tensor
        [k, 4] that is used as it is, unvalidated (the kernel clamps each value into [0, N]; left > right or top > bottom is an
        empty box); None = THE WHOLE BOARD, the
        reference's nullptr -- not the bounding box that None means for life_map and ld_read.  A row whose slot id lies outside
        the pool gets zeros."""
        t, p, k = self._ids(ids, n)
        reg = self._boxes(regions, k, device_ok=True)
        np_ = self.n * self.n
        cand = torch.empty((k, np_), dtype=torch.uint8, device=self.device)
        valid = torch.empty((k, np_), dtype=torch.uint8, device=self.device)
        groups = torch.empty((k, np_), dtype=torch.uint8, device=self.device)
        check(self.L.elfgo_region_moves(self._h, p, k, C.c_void_p(reg.data_ptr()) if reg is not None else None, int(self_atari_thres),
                                        C.c_void_p(cand.data_ptr()), C.c_void_p(valid.data_ptr()), C.c_void_p(groups.data_ptr()),
                                        self._stream()))
        return cand, valid, groups

    def ld_read(self, seeds, ids=None, regions=None, playouts=256, self_atari_thres=3, attackers=None, max_steps=1 << 20, max_lanes=0):
        """Life-and-death reading by region playouts (elfgo_ld_run) -> LdReading.  Per row: `playouts` playouts from a private
        copy of the slot, playout k with seed seeds[i] + k * 0x9E3779B97F4A7C15 (mod 2^64), moves drawn from
        FindAllCandidateMovesInRegion(board, box, next_player, self_atari_thres), each judged where it ends by
        OneGroupLives(defender, box) and by the defender's stones left inside the box.  self_atari_thres defaults to 3: with 1
        the attacker may not throw in, and the reading is blind to most killing moves.
        regions: k host boxes as for life_map (ValueError before anything is launched) or a device int32 tensor [k, 4] used as it
        is, unvalidated (clamped by the kernel; left > right or top > bottom is an empty box); None = getBoardBBox of each row.
        attackers: per row 1 (Black) / 2 (White), anything else = GuessLDAttacker(box); None = guess every row.
        The scratch handle is ownership()'s.  Unlike playout(), this works on a track_placed engine too: playout() raises there
        because it plays on the slots without the placement table, while ld_read only reads the slots -- every playout runs on a
        private copy -- so the table stays true."""
        sd, t, p, k = self._seeds(seeds, ids)
        reg = self._boxes(regions, k, device_ok=True)
        att = None
        if attackers is not None:
            att = torch.as_tensor(attackers, dtype=torch.uint8, device=self.device).reshape(-1).contiguous()
            if att.numel() != k:
                raise ValueError("attackers must hold one colour per row (%d), got %d" % (k, att.numel()))
        own = self._own_handle(max_lanes)
        na = self.n * self.n + 1
        info = torch.empty((k, 8), dtype=torch.int32, device=self.device)
        stats = torch.empty((k, 8), dtype=torch.int64, device=self.device)
        first = torch.empty((k, 3, na), dtype=torch.int32, device=self.device)
        check(self.L.elfgo_ld_run(own[1], p, C.c_void_p(sd.data_ptr()), k, int(playouts), int(max_steps), int(self_atari_thres),
                                  C.c_void_p(reg.data_ptr()) if reg is not None else None,
                                  C.c_void_p(att.data_ptr()) if att is not None else None, C.c_void_p(info.data_ptr()),
                                  C.c_void_p(stats.data_ptr()), C.c_void_p(first.data_ptr()), self._stream()))
        return LdReading(self.n, int(playouts), info, stats, first)
