"""TEST INFRASTRUCTURE ONLY: ctypes bindings for the two CPU checkers.

* ``Port(n)``  -> oracle/libgo_oracle{n}.so  (C restatement, oracle/go_oracle.c; travels as source)
* ``Ref(n)``   -> oracle/_ref/libelfref{n}.so (the real reference compiled in place against the stand-in headers of
                  oracle/shim; prebuilt .so travels to the GPU box, sources never enter this repo)
* ``RefBoard(n)`` -> oracle/_ref/libelfboard{n}.so (the reference's board engine alone, base/board.cc + base/common.cc, built
                  with NO stand-in on the include path: evidence that shares no header with ``Ref``)

Both expose the same small interface so tests can run one move list through either.
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ZOBRIST_BIN = os.path.join(HERE, "..", "elf_amd", "data", "zobrist21.bin")

M_PASS, M_RESIGN, M_SKIP, M_INVALID, M_CLEAR = 0, 1, 2, 3, 4
S_EMPTY, S_BLACK, S_WHITE, S_OFF = 0, 1, 2, 3


def coord(n, x, y):
    """base/board.h:183-184 OFFSETXY"""
    return (y + 1) * (n + 2) + (x + 1)


def playout_seeds(n_boards, base=0):
    """seed s_b = 0x9E3779B9*b + 1"""
    b = np.arange(base, base + n_boards, dtype=np.uint64)
    return b * np.uint64(0x9E3779B9) + np.uint64(1)


class _Engine:
    prefix = ""

    def __init__(self, lib, n):
        self.L = lib
        self.n = n
        p = self.prefix
        vp = C.c_void_p

        def fn(name, res, *args):
            f = getattr(lib, p + name)
            f.restype = res
            f.argtypes = list(args)
            return f

        self._new = fn("new", vp)
        self._free = fn("free", None, vp)
        self._reset = fn("reset", None, vp)
        self._clone = fn("clone", vp, vp)
        self._forward = fn("forward", C.c_int, vp, C.c_int)
        self._check = fn("check_move", C.c_int, vp, C.c_int)
        self._term = fn("terminated", C.c_int, vp)
        self._hash = fn("hash", C.c_uint64, vp)
        self._eval = fn("evaluate", C.c_float, vp, C.c_float)
        self._info = fn("info", None, vp, vp)
        self._mask = fn("legal_mask", None, vp, vp)
        self._board = fn("board", None, vp, vp, vp)
        self._agz = fn("extract_agz", None, vp, C.c_int, vp)
        self._eye = fn("is_true_eye", C.c_int, vp, C.c_int, C.c_int)
        self._pm = fn("playout_moves", C.c_int, vp, C.c_uint64, C.c_int, vp)

    # --- state handles
    def new(self):
        return self._new()

    def free(self, s):
        self._free(s)

    def reset(self, s):
        self._reset(s)

    def clone(self, s):
        return self._clone(s)

    def forward(self, s, c):
        return self._forward(s, int(c))

    def check_move(self, s, c):
        return self._check(s, int(c))

    def terminated(self, s):
        return bool(self._term(s))

    def hash(self, s):
        return int(self._hash(s))

    def evaluate(self, s, komi):
        return float(self._eval(s, komi))

    def info(self, s):
        a = np.zeros(10, np.int32)
        self._info(s, a.ctypes.data)
        return a

    def legal_mask(self, s):
        a = np.zeros(self.n * self.n + 1, np.uint8)
        self._mask(s, a.ctypes.data)
        return a

    def board(self, s):
        col = np.zeros(self.n * self.n, np.uint8)
        lib = np.zeros(self.n * self.n, np.int16)
        self._board(s, col.ctypes.data, lib.ctypes.data)
        return col, lib

    def extract_agz(self, s, d4):
        a = np.zeros((18, self.n, self.n), np.float32)
        self._agz(s, int(d4), a.ctypes.data)
        return a

    def is_true_eye(self, s, c, player):
        return bool(self._eye(s, int(c), int(player)))

    def true_eye_mask(self, s, player):
        """is_true_eye of every point for `player`, action order (x*n + y)"""
        n = self.n
        a = np.zeros(n * n, np.uint8)
        f = getattr(self.L, self.prefix + "true_eye_mask", None)
        if f is not None:
            f.restype = None
            f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            f(s, int(player), a.ctypes.data)
        else:
            for x in range(n):
                for y in range(n):
                    a[x * n + y] = self._eye(s, (y + 1) * (n + 2) + x + 1, int(player))
        return a

    def playout_moves(self, s, seed, max_steps=100000):
        mv = np.zeros(2 * self.n * self.n + 8, np.int32)
        k = self._pm(s, C.c_uint64(int(seed)), int(max_steps), mv.ctypes.data)
        return mv[:k].copy()


class Port(_Engine):
    prefix = "orc_"

    def __init__(self, n=19):
        path = os.path.join(HERE, "libgo_oracle%d.so" % n)
        lib = C.CDLL(path)
        super().__init__(lib, n)
        z = np.fromfile(ZOBRIST_BIN, dtype=np.uint64)
        assert z.size == 441
        zz = np.zeros((n + 2) * (n + 2), np.uint64)
        zz[:] = z[: zz.size]  # hash_num.h:12 is indexed by Coord; 9x9 uses the first 121 entries
        lib.orc_set_zobrist.argtypes = [C.c_void_p]
        lib.orc_set_zobrist(zz.ctypes.data)
        lib.orc_coord2action.restype = C.c_int64
        lib.orc_coord2action.argtypes = [C.c_int, C.c_int]
        lib.orc_action2coord.restype = C.c_int
        lib.orc_action2coord.argtypes = [C.c_int, C.c_int64]

    def coord2action(self, d4, c):
        return int(self.L.orc_coord2action(int(d4), int(c)))

    def action2coord(self, d4, a):
        return int(self.L.orc_action2coord(int(d4), int(a)))


class Ref(_Engine):
    prefix = "ref_"

    @staticmethod
    def path(n):
        return os.path.join(HERE, "_ref", "libelfref%d.so" % n)

    @staticmethod
    def available(n=19):
        return os.path.exists(Ref.path(n))

    def __init__(self, n=19):
        lib = C.CDLL(Ref.path(n))
        super().__init__(lib, n)
        lib.ref_coord2action.restype = C.c_int64
        lib.ref_coord2action.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.ref_action2coord.restype = C.c_int
        lib.ref_action2coord.argtypes = [C.c_void_p, C.c_int, C.c_int64]
        lib.ref_playout.restype = C.c_int64
        lib.ref_playout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.ref_sgf_moves.restype = C.c_int
        lib.ref_sgf_moves.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
        self._tmp = self.new()

    def coord2action(self, d4, c):
        return int(self.L.ref_coord2action(self._tmp, int(d4), int(c)))

    def action2coord(self, d4, a):
        return int(self.L.ref_action2coord(self._tmp, int(d4), int(a)))

    def playout(self, seeds, max_steps=100000, threads=1, with_feat=False):
        """config-2 protocol, multi-threaded; returns (total_steps, out[n,4]=hash_lo,hash_hi,ply,steps)"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        out = np.zeros((seeds.size, 4), np.uint32)
        tot = self.L.ref_playout(seeds.ctypes.data, seeds.size, int(max_steps), int(threads), int(with_feat), out.ctypes.data)
        return int(tot), out

    def sgf_moves(self, path):
        mv = np.zeros(2048, np.int32)
        pl = np.zeros(2048, np.int32)
        k = self.L.ref_sgf_moves(path.encode(), mv.ctypes.data, pl.ctypes.data, 2048)
        if k < 0:
            raise IOError(path)
        return mv[:k].copy(), pl[:k].copy()

    def sgf_parse(self, text):
        """Sgf::load(filename, game_string) -> (moves, players, dict(size, komi, handi, winner, win_margin)) or None (load failed)"""
        mv = np.zeros(4096, np.int32)
        pl = np.zeros(4096, np.int32)
        h = np.zeros(5, np.float32)
        k = self.L.ref_sgf_parse(C.c_char_p(text.encode("latin-1")), mv.ctypes.data_as(C.c_void_p), pl.ctypes.data_as(C.c_void_p), C.c_int(4096),
                                 h.ctypes.data_as(C.c_void_p))
        if k < 0:
            return None
        return mv[:k].copy(), pl[:k].copy(), dict(size=int(h[0]), komi=float(h[1]), handi=int(h[2]), winner=int(h[3]), win_margin=float(h[4]))

    def zobrist(self):
        z = np.zeros((self.n + 2) ** 2, np.uint64)
        self.L.ref_zobrist.argtypes = [C.c_void_p]
        self.L.ref_zobrist(z.ctypes.data)
        return z


class RefBoard:
    """The reference's board engine with no stand-in header anywhere in its build (oracle/ref_board_capi.cc over base/board.cc +
    base/common.cc).  A handle is a plain Board: play() is TryPlay2 + Play, which is all GoState::forward does to its board;
    super-ko, the move limit and `terminated` are GoState-level and do not exist here."""

    @staticmethod
    def path(n):
        return os.path.join(HERE, "_ref", "libelfboard%d.so" % n)

    @staticmethod
    def available(n=19):
        return os.path.exists(RefBoard.path(n))

    def __init__(self, n=19):
        self.n = n
        L = self.L = C.CDLL(RefBoard.path(n))
        vp = C.c_void_p
        for name, res, args in (("new", vp, []), ("free", None, [vp]), ("reset", None, [vp]), ("clone", vp, [vp]),
                                ("play", C.c_int, [vp, C.c_int]), ("try_play", C.c_int, [vp, C.c_int]), ("hash", C.c_uint64, [vp]),
                                ("info", None, [vp, vp]), ("board", None, [vp, vp, vp]), ("legal_mask", None, [vp, vp]),
                                ("true_eye_mask", None, [vp, C.c_int, vp]), ("is_true_eye", C.c_int, [vp, C.c_int, C.c_int]),
                                ("is_game_end", C.c_int, [vp]), ("valid_moves", C.c_int, [vp, C.c_int, vp]),
                                ("replay", C.c_int, [vp, vp, C.c_int] + [vp] * 8), ("board_size", C.c_int, [])):
            f = getattr(L, "rb_" + name)
            f.restype, f.argtypes = res, args
        assert L.rb_board_size() == n

    def new(self):
        return self.L.rb_new()

    def free(self, b):
        self.L.rb_free(b)

    def reset(self, b):
        self.L.rb_reset(b)

    def clone(self, b):
        return self.L.rb_clone(b)

    def play(self, b, c):
        """TryPlay2 then Play; the TryPlay2 result"""
        return self.L.rb_play(b, int(c))

    def try_play(self, b, c):
        return self.L.rb_try_play(b, int(c))

    def hash(self, b):
        return int(self.L.rb_hash(b))

    def info(self, b):
        a = np.zeros(10, np.int32)
        self.L.rb_info(b, a.ctypes.data)
        return a

    def board(self, b):
        col = np.zeros(self.n * self.n, np.uint8)
        lib = np.zeros(self.n * self.n, np.int16)
        self.L.rb_board(b, col.ctypes.data, lib.ctypes.data)
        return col, lib

    def legal_mask(self, b):
        a = np.zeros(self.n * self.n + 1, np.uint8)
        self.L.rb_legal_mask(b, a.ctypes.data)
        return a

    def true_eye_mask(self, b, player):
        a = np.zeros(self.n * self.n, np.uint8)
        self.L.rb_true_eye_mask(b, int(player), a.ctypes.data)
        return a

    def is_true_eye(self, b, c, player):
        return bool(self.L.rb_is_true_eye(b, int(c), int(player)))

    def is_game_end(self, b):
        return bool(self.L.rb_is_game_end(b))

    def valid_moves(self, b, player):
        """FindAllValidMoves for `player`, in that function's own order (Coords)"""
        a = np.zeros(self.n * self.n, np.int32)
        k = self.L.rb_valid_moves(b, int(player), a.ctypes.data)
        return a[:k].copy()

    def replay(self, moves, b=None):
        """One call per game: plays `moves` from `b` (a fresh board when None, freed afterwards) and returns the arrays of all
        len(moves) + 1 positions (row 0 = before the first move): dict(ok [k], hash [k+1] u64, info [k+1,10], colour, libs
        [k+1,n*n], legal [k+1,n*n+1], eyes [k+1,2,n*n] (Black's, White's), game_end [k+1])"""
        mv = np.ascontiguousarray(moves, dtype=np.int32)
        k, p = mv.size, self.n * self.n
        out = dict(ok=np.zeros(k, np.uint8), hash=np.zeros(k + 1, np.uint64), info=np.zeros((k + 1, 10), np.int32),
                   colour=np.zeros((k + 1, p), np.uint8), libs=np.zeros((k + 1, p), np.int16), legal=np.zeros((k + 1, p + 1), np.uint8),
                   eyes=np.zeros((k + 1, 2, p), np.uint8), game_end=np.zeros(k + 1, np.uint8))
        own = b is None
        if own:
            b = self.new()
        self.L.rb_replay(b, mv.ctypes.data, k, *[out[f].ctypes.data for f in ("ok", "hash", "info", "colour", "libs", "legal", "eyes", "game_end")])
        if own:
            self.free(b)
        return out


# ---- MCTS / self-play: the real reference stack (oracle/ref_selfplay.cc) and the stub net ----------------
class RefSpConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_games", "batchsize", "mcts_threads", "rollouts_per_thread", "rollouts_per_batch",
                                         "virtual_loss", "persistent_tree", "use_prior", "unexplored_q_zero",
                                         "root_unexplored_q_zero")] + \
        [("c_puct", C.c_float), ("root_epsilon", C.c_float), ("root_alpha", C.c_float), ("seed", C.c_uint32), ("komi", C.c_float),
         ("ply_pass_enabled", C.c_int32), ("policy_distri_cutoff", C.c_int32), ("move_cutoff", C.c_int32),
         ("resign_thres", C.c_float), ("never_resign_prob", C.c_float), ("net_salt", C.c_uint32), ("net_tie_levels", C.c_int32),
         ("max_searches", C.c_int32), ("timeout_usec", C.c_int32),
         # round 3 (read by oracle/ref_selfplay.cc only; the CPU restatement plays one AI per game)
         ("black_ver", C.c_int32), ("white_ver", C.c_int32), ("player_swap", C.c_int32), ("white_puct", C.c_float),
         ("white_rollouts_per_batch", C.c_int32), ("white_rollouts_per_thread", C.c_int32), ("white_net_salt", C.c_uint32),
         ("pick_method", C.c_int32), ("black_policy_only", C.c_int32), ("white_policy_only", C.c_int32), ("thread_used", C.c_int32),
         ("req2_after_searches", C.c_int32), ("req2_black_ver", C.c_int32), ("req2_async", C.c_int32),
         ("cheat_eval_new_model_wins_half", C.c_int32), ("cheat_selfplay_random_result", C.c_int32),
         ("online", C.c_int32), ("following_pass", C.c_int32), ("net_value_on", C.c_int32), ("net_value", C.c_float),
         ("req2_ts", C.c_int32), ("req2_rollouts_per_thread", C.c_int32), ("req2_rollouts_per_batch", C.c_int32), ("req2_c_puct", C.c_float),
         ("req2_root_epsilon", C.c_float), ("req2_root_alpha", C.c_float), ("req2_unexplored_q_zero", C.c_int32),
         ("req2_root_unexplored_q_zero", C.c_int32), ("req2_white_ver", C.c_int32)]


class RefSpSearch(C.Structure):
    _fields_ = [("game", C.c_int32), ("move_played", C.c_int32), ("best_action", C.c_int32), ("total_visits", C.c_int32),
                ("n_edges", C.c_int32), ("root_value", C.c_float), ("max_score", C.c_float), ("pad", C.c_int32)]


MCTS_DEFAULTS = dict(num_games=1, batchsize=16, mcts_threads=1, rollouts_per_thread=8192, rollouts_per_batch=16, virtual_loss=1,
                     persistent_tree=1, use_prior=1, unexplored_q_zero=0, root_unexplored_q_zero=0, c_puct=1.5, root_epsilon=0.25,
                     root_alpha=0.03, seed=1234, komi=7.5, ply_pass_enabled=0, policy_distri_cutoff=0, move_cutoff=-1,
                     resign_thres=0.0, never_resign_prob=0.0, net_salt=7, net_tie_levels=0, max_searches=4, timeout_usec=10,
                     black_ver=0, white_ver=-1, player_swap=0, white_puct=-1.0, white_rollouts_per_batch=-1,
                     white_rollouts_per_thread=-1, white_net_salt=8, pick_method=0, black_policy_only=0, white_policy_only=0,
                     thread_used=0, req2_after_searches=0, req2_black_ver=0, req2_async=0,
                     cheat_eval_new_model_wins_half=0, cheat_selfplay_random_result=0, online=0, following_pass=0, net_value_on=0,
                     net_value=0.0, req2_ts=0, req2_rollouts_per_thread=0, req2_rollouts_per_batch=0, req2_c_puct=0.0, req2_root_epsilon=0.0,
                     req2_root_alpha=0.0, req2_unexplored_q_zero=0, req2_root_unexplored_q_zero=0, req2_white_ver=-1)


class RefSelfPlay:
    """The reference's own Context + GoGameSelfPlay + MCTSGoAI, net = stub (or a Python callback)."""

    @staticmethod
    def path(n, turnstile=False, canonical_backup=False):
        sfx = "_tsh2" if (turnstile and canonical_backup) else "_ts" if turnstile else "_h2" if canonical_backup else ""
        return os.path.join(HERE, "_ref", "libelfsp%d%s.so" % (n, sfx))

    @classmethod
    def available(cls, n, turnstile=False, canonical_backup=False):
        return os.path.exists(cls.path(n, turnstile, canonical_backup))

    def __init__(self, n, turnstile=False, canonical_backup=False):
        """turnstile=True: the build whose copy of tree_search.h carries the four elf_ts_hook() calls (oracle/Makefile), with the
        turnstile switched on: the search threads of a game take turns in thread order (mcts_threads > 1 becomes deterministic)"""
        self.n = n
        self.na = n * n + 1
        self.L = C.CDLL(self.path(n, turnstile, canonical_backup))
        self.L.refsp_run.restype = C.c_int
        self.turnstile = bool(turnstile)
        # canonical_backup=True: the build whose batch_rollouts backs the unique leaves of a batch up in first-occurrence order
        # instead of heap-address order (oracle/Makefile, libelfsp*_h2.so)
        assert self.L.refsp_has_canonical_backup() == (1 if canonical_backup else 0)
        if turnstile:
            assert self.L.refsp_has_turnstile() == 1
            self.L.refsp_set_turnstile(C.c_int(1))

    def run(self, net=None, human_script=None, **kw):
        """-> dict(search=list[RefSpSearch], coord, visits, prior, reward [k, NA], stats); online=1 with human_script = the answers
        ("a") to the human_actor prompts additionally gives prompts [p, 18, n, n] uint8"""
        cfg = dict(MCTS_DEFAULTS)
        cfg.update(kw)
        c = RefSpConfig(**cfg)
        hs = np.ascontiguousarray(human_script if human_script is not None else [], np.int64)
        self.L.refsp_set_human_script(hs.ctypes.data_as(C.c_void_p), C.c_int(hs.size))
        m, na = c.max_searches, self.na
        S = (RefSpSearch * m)()
        coord = np.full((m, na), -1, np.int32); visits = np.zeros((m, na), np.int32)
        prior = np.zeros((m, na), np.float32); reward = np.zeros((m, na), np.float32)
        stats = (C.c_int64 * 3)()
        cb = None
        if net is not None:
            NETFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
            n = self.n

            def _net(sp, b, pip, vp, _u):
                s = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_float)), shape=(b, 18, n, n))
                pi, v = net(s)
                np.ctypeslib.as_array(C.cast(pip, C.POINTER(C.c_float)), shape=(b, na))[:] = pi
                np.ctypeslib.as_array(C.cast(vp, C.POINTER(C.c_float)), shape=(b,))[:] = v
            cb = NETFN(_net)
        k = self.L.refsp_run(C.byref(c), cb, None, S, coord.ctypes.data_as(C.c_void_p), visits.ctypes.data_as(C.c_void_p),
                             prior.ctypes.data_as(C.c_void_p), reward.ctypes.data_as(C.c_void_p), stats)
        if k < 0:
            raise RuntimeError("refsp_run failed")
        self.L.refsp_white_rows.restype = C.c_int64
        self.L.refsp_game_starts.restype = C.c_int64
        vers8 = (C.c_int64 * 8)()
        starts = int(self.L.refsp_game_starts(vers8))
        self.L.refsp_last_prompts.restype = C.c_int64
        npr = int(self.L.refsp_last_prompts(None, C.c_int64(0)))
        prompts = np.zeros((npr, 18, self.n, self.n), np.uint8)
        if npr:
            self.L.refsp_last_prompts(prompts.ctypes.data_as(C.c_void_p), C.c_int64(prompts.size))
        return dict(search=list(S)[:k], coord=coord[:k], visits=visits[:k], prior=prior[:k], reward=reward[:k], prompts=prompts,
                    batches=int(stats[0]), rows=int(stats[1]), usec=int(stats[2]), records=self.last_records(),
                    white_rows=int(self.L.refsp_white_rows()), game_starts=starts, start_versions=[int(v) for v in vers8][:min(starts, 8)])

    # ---- records (GoStateExt::dumpRecord) and the trainer's extractors (GoStateExtOffline + GoFeature)
    def _text(self, fn, *args):
        fn.restype = C.c_int64
        n = fn(*args, None, C.c_int64(0))
        if n < 0:
            raise RuntimeError("reference threw")
        buf = C.create_string_buffer(int(n) + 1)
        fn(*args, buf, C.c_int64(n))
        return buf.raw[:n].decode()

    def set_time(self, t):
        """the value the reference's time(NULL) returns (seed of MCTSResultT::addActions' static uniform_random generator): set it
        before the first search of the process"""
        self.L.refsp_set_time(C.c_int64(int(t)))

    def set_preload(self, path, move_to=-1):
        """GameOptions.preload_sgf / preload_sgf_move_to for the following run() calls ("" = off)"""
        self.L.refsp_set_preload(C.c_char_p((path or "").encode()), C.c_int(move_to))

    def last_records(self):
        """JSON array text: Record of every game that finished during the last run()"""
        return self._text(self.L.refsp_last_records)

    def last_sgfs(self):
        """GoStateExt::dumpSgf of every game that finished during the last run() (what dump_record_prefix writes), list of texts"""
        import json
        return json.loads(self._text(self.L.refsp_last_sgfs))

    def record_roundtrip(self, record_json):
        return self._text(self.L.reftrain_record_roundtrip, record_json.encode())

    def sgfstr2coords(self, sgf):
        out = np.zeros(4096, np.uint16)
        k = self.L.reftrain_sgfstr2coords(sgf.encode(), out.ctypes.data_as(C.c_void_p), 4096)
        return out[:k].copy()

    def coords2sgfstr(self, coords):
        c = np.ascontiguousarray(coords, dtype=np.uint16)
        return self._text(self.L.reftrain_coords2sgfstr, c.ctypes.data_as(C.c_void_p), C.c_int(c.size))

    def train_bench(self, records_json_array, n_samples, threads, num_future_actions=1):
        """-> (board steps replayed, seconds): GoGameTrain::act's per-sample work on `threads` host threads"""
        sec = C.c_double(0)
        self.L.reftrain_bench.restype = C.c_int64
        st = self.L.reftrain_bench(records_json_array.encode(), C.c_int(n_samples), C.c_int(threads), C.c_int(num_future_actions),
                                   C.byref(sec))
        if st < 0:
            raise RuntimeError("reftrain_bench failed")
        return int(st), float(sec.value)

    def train_sample(self, record_json, move_to, d4, num_future_actions=1):
        """The reference's "train" batch row for (record, move_to, d4): dict of numpy arrays"""
        n, na = self.n, self.na
        s = np.zeros((18, n, n), np.float32); oa = np.zeros(num_future_actions, np.int64)
        ms = np.zeros(na, np.float32)
        w = C.c_float(); pv = C.c_float(); mi = C.c_int32(); nm = C.c_int32(); ac = C.c_int32(); sv = C.c_int64()
        rc = self.L.reftrain_sample(record_json.encode(), C.c_int(move_to), C.c_int(d4), C.c_int(num_future_actions),
                                    s.ctypes.data_as(C.c_void_p), oa.ctypes.data_as(C.c_void_p), C.byref(w),
                                    ms.ctypes.data_as(C.c_void_p), C.byref(pv), C.byref(mi), C.byref(nm), C.byref(ac), C.byref(sv))
        if rc != 0:
            raise RuntimeError("reftrain_sample failed")
        return dict(s=s, offline_a=oa, winner=np.float32(w.value), mcts_scores=ms, predicted_value=np.float32(pv.value),
                    move_idx=mi.value, num_move=nm.value, aug_code=ac.value, selfplay_ver=sv.value)


    # ---- the client's wire formats: the real Records / MsgRequestSeq (oracle/ref_selfplay.cc refrec_*)
    def _text(self, fn, *args):
        fn.restype = C.c_int64
        n = int(fn(*args, None, C.c_int64(0)))
        if n < 0:
            return None
        buf = C.create_string_buffer(n + 1)
        fn(*args, buf, C.c_int64(n + 1))
        return buf.raw[:n].decode("latin-1")

    def client_reset(self, identity):
        self.L.refrec_client_reset(identity.encode())

    def client_feed(self, record_json):
        assert self.L.refrec_client_feed(record_json.encode("latin-1")) == 0

    def client_update_state(self, thread_id, seq, move_idx, black, white):
        self.L.refrec_client_update_state(C.c_int(thread_id), C.c_int(seq), C.c_int(move_idx), C.c_int64(black), C.c_int64(white))

    def client_dump(self, cap=1 << 24):
        """GuardedRecords::dumpAndClear"""
        self.L.refrec_client_dump_and_clear.restype = C.c_int64
        buf = C.create_string_buffer(cap)
        n = int(self.L.refrec_client_dump_and_clear(buf, C.c_int64(cap)))
        assert 0 <= n < cap
        return buf.raw[:n].decode("latin-1")

    def records_parse(self, text):
        """the server's Records::createFromJsonString -> (records, states, sum of move_idx, identity) or None if it throws"""
        out3 = (C.c_int64 * 3)()
        self.L.refrec_records_parse.restype = C.c_int64
        buf = C.create_string_buffer(4096)
        n = int(self.L.refrec_records_parse(text.encode("latin-1"), out3, buf, C.c_int64(4096)))
        if n < 0:
            return None
        return int(out3[0]), int(out3[1]), int(out3[2]), buf.raw[:n].decode("latin-1")

    def request_seq_dump(self, black_ver, white_ver, client_type=1, num_game_thread_used=-1, black_thres=0.0, white_thres=0.0,
                         never_resign_prob=0.0, player_swap=0, async_=0, seq=0, **kw):
        """MsgRequestSeq::dumpJsonString, TSOptions from the MCTS_DEFAULTS-style keywords"""
        cfg = dict(MCTS_DEFAULTS)
        cfg.update(kw)
        c = RefSpConfig(**cfg)
        return self._text(self.L.refrec_request_seq_dump, C.byref(c), C.c_int64(black_ver), C.c_int64(white_ver), C.c_int(client_type),
                          C.c_int(num_game_thread_used), C.c_float(black_thres), C.c_float(white_thres), C.c_float(never_resign_prob),
                          C.c_int(player_swap), C.c_int(async_), C.c_int64(seq))

    def request_seq_roundtrip(self, text):
        """text -> MsgRequestSeq -> text, None when the reference throws"""
        return self._text(self.L.refrec_request_seq_roundtrip, text.encode("latin-1"))

    def train_act(self, records, num_reader=4, q_min_size=1, q_max_size=1000, insert_seed=1, game_seed=7, num_acts=2, num_future_actions=1):
        """The reference's trainer input path end to end (oracle/ref_selfplay.cc reftrain_act): records (list of Record JSON texts)
        inserted into a ReaderQueuesT<Record> with InsertWithParity, one real GoGameTrain thread, num_acts "train" batches of 64
        rows -> dict of arrays [num_acts * 64, ...]"""
        n, na, rows = self.n, self.na, 64 * num_acts
        s = np.zeros((rows, 18, n, n), np.uint8); oa = np.zeros((rows, num_future_actions), np.int64)
        w = np.zeros(rows, np.float32); ms = np.zeros((rows, na), np.float32)
        mi = np.zeros(rows, np.int32); nm = np.zeros(rows, np.int32); ac = np.zeros(rows, np.int32); sv = np.zeros(rows, np.int64)
        text = "[" + ",".join(records) + "]"
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self.L.reftrain_act(text.encode(), C.c_int(num_reader), C.c_int(q_min_size), C.c_int(q_max_size), C.c_uint32(insert_seed),
                                 C.c_int64(game_seed), C.c_int(num_acts), C.c_int(num_future_actions), p(s), p(oa), p(w), p(ms), p(mi), p(nm),
                                 p(ac), p(sv))
        if rc != rows:
            raise RuntimeError("reftrain_act failed (%d)" % rc)
        return dict(s=s, offline_a=oa, winner=w, mcts_scores=ms, move_idx=mi, num_move=nm, aug_code=ac, selfplay_ver=sv)


class PortSelfPlay:
    """The CPU restatement of the search + self-play loop (oracle/mcts_oracle.cc over go_oracle.c); same run() interface and
    result layout as RefSelfPlay, which it is pinned against (tests/test_oracle_mcts.py)."""

    def __init__(self, n):
        self.n = n
        self.na = n * n + 1
        Port(n)   # loads the library's Zobrist table
        self.L = C.CDLL(os.path.join(HERE, "libgo_oracle%d.so" % n))
        self.L.orcsp_run.restype = C.c_int

    def set_time(self, t):
        self.L.orcsp_set_time(C.c_int64(int(t)))

    def set_preload(self, moves, move_to=-1):
        """GameOptions.preload_sgf as Coords for the following run() calls (empty = off)"""
        mv = np.ascontiguousarray(moves, dtype=np.uint16)
        self.L.orcsp_set_preload(mv.ctypes.data_as(C.c_void_p), C.c_int(mv.size), C.c_int(move_to))

    def run(self, net=None, **kw):
        cfg = dict(MCTS_DEFAULTS)
        cfg.update(kw)
        c = RefSpConfig(**cfg)
        m, na = c.max_searches, self.na
        S = (RefSpSearch * m)()
        coord = np.full((m, na), -1, np.int32); visits = np.zeros((m, na), np.int32)
        prior = np.zeros((m, na), np.float32); reward = np.zeros((m, na), np.float32)
        stats = (C.c_int64 * 3)()
        cb = None
        if net is not None:      # a Python net instead of the stub: net(s [b,18,n,n]) -> (pi [b,na], v [b])
            NETFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
            n = self.n

            def _net(sp, b, pip, vp, _u):
                s = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_float)), shape=(b, 18, n, n))
                pi, v = net(s)
                np.ctypeslib.as_array(C.cast(pip, C.POINTER(C.c_float)), shape=(b, na))[:] = pi
                np.ctypeslib.as_array(C.cast(vp, C.POINTER(C.c_float)), shape=(b,))[:] = v
            cb = NETFN(_net)
        k = self.L.orcsp_run(C.byref(c), cb, None, S, coord.ctypes.data_as(C.c_void_p), visits.ctypes.data_as(C.c_void_p),
                             prior.ctypes.data_as(C.c_void_p), reward.ctypes.data_as(C.c_void_p), stats)
        if k < 0:
            raise RuntimeError("orcsp_run failed: %d" % k)
        return dict(search=list(S)[:k], coord=coord[:k], visits=visits[:k], prior=prior[:k], reward=reward[:k],
                    batches=int(stats[0]), rows=int(stats[1]))


def stub_net(n, s, salt=7, tie_levels=0):
    """oracle/stub_net.h through the port library: s [B,18,n,n] f32 -> (pi [B,n*n+1], v [B])"""
    L = C.CDLL(os.path.join(HERE, "libgo_oracle%d.so" % n))
    s = np.ascontiguousarray(s, dtype=np.float32)
    b = s.shape[0]
    pi = np.zeros((b, n * n + 1), np.float32)
    v = np.zeros((b,), np.float32)
    L.orc_stub_net(s.ctypes.data_as(C.c_void_p), C.c_int(b), C.c_uint32(salt), C.c_int(tie_levels), pi.ctypes.data_as(C.c_void_p),
                   v.ctypes.data_as(C.c_void_p))
    return pi, v


# ---- trainer side: CPU restatement of the "train" batch row (checker for tests; pinned on tests/golden/train_*.npz) -------
def sgfstr2coords(n, sgf):
    """sgfstr2coords + str2coord (sgf/sgf.h:21-46,97-125)"""
    S, out = n + 2, []
    if not sgf or sgf[0] != "(":
        return np.zeros(0, np.uint16)
    i = 1
    while True:
        if i >= len(sgf) or sgf[i] != ";":
            break
        while i < len(sgf) and sgf[i] != "[":
            i += 1
        if i == len(sgf):
            break
        i += 1
        j = i
        while j < len(sgf) and sgf[j] != "]":
            j += 1
        if j == len(sgf):
            break
        s = sgf[i:j]
        if len(s) < 2:
            c = 0
        else:
            t = [ch for ch in s if ch not in "\n "]
            k = 0
            while k < len(s) and s[k] in "\n ":
                k += 1
            if k == len(s):
                c = 3
            else:
                x = ord(s[k]) - 97
                k += 1
                while k < len(s) and s[k] in "\n ":
                    k += 1
                if k == len(s):
                    c = 3
                else:
                    y = ord(s[k]) - 97
                    c = (y + 1) * S + (x + 1) if (0 <= x < n and 0 <= y < n) else 3
            del t
        out.append(c)
        i = j + 1
    return np.array(out, np.uint16)


def coord2action(n, c, d4):
    """BoardFeature::coord2Action (board_feature.h:132-137) with Transform (:97-113)"""
    S = n + 2
    if c == 0:
        return n * n
    x, y = c % S - 1, c // S - 1
    rot = d4 % 4
    if rot == 1:
        x, y = y, n - x - 1
    elif rot == 2:
        x, y = n - x - 1, n - y - 1
    elif rot == 3:
        x, y = n - y - 1, x
    if (d4 >> 2) == 1:
        x, y = y, x
    return x * n + y


def action2coord(n, a, d4):
    """BoardFeature::action2Coord (board_feature.h:139-144) with InvTransform (:115-130)"""
    S = n + 2
    if a == -1 or a == n * n:
        return 0
    x, y = a // n, a % n
    if (d4 >> 2) == 1:
        x, y = y, x
    rot = d4 % 4
    if rot == 1:
        x, y = n - y - 1, x
    elif rot == 2:
        x, y = n - x - 1, n - y - 1
    elif rot == 3:
        x, y = y, n - x - 1
    return (y + 1) * S + (x + 1)


def port_train_sample(port, record, move_to, d4, nfa=1):
    """Restatement of GoStateExtOffline::fromRecord + switchBeforeMove (go_state_ext.h:248-290) and the GoFeature "train"
    extractors (game_feature.h:73-145) over the C port of the board engine.  record: parsed Record dict."""
    n = port.n
    res = record["result"]
    mv = sgfstr2coords(n, res["content"])
    st = port.new()
    for c in mv[:move_to]:
        if int(c) != 3:
            port.forward(st, int(c))
    idx = int(port.info(st)[0]) - 1
    out = dict(s=port.extract_agz(st, d4), move_idx=idx, num_move=len(mv), aug_code=d4,
               winner=np.float32(1.0 if res["reward"] > 0 else -1.0), selfplay_ver=int(record["request"]["vers"]["black_ver"]))
    port.free(st)
    vals = res["values"]
    out["predicted_value"] = np.float32(vals[idx]) if idx < len(vals) else np.float32(0)
    out["offline_a"] = np.array([coord2action(n, int(mv[idx + j]), d4) for j in range(nfa)], np.int64)
    ms = np.zeros(n * n + 1, np.float32)
    pol = res.get("policies") or []
    if idx < len(pol):
        p = pol[idx]
        for a in range(n * n + 1):
            ms[a] = p[action2coord(n, a, d4)]
        with np.errstate(invalid="ignore", divide="ignore"):
            ms = ms / ms.sum(dtype=np.float32)
    else:
        ms[coord2action(n, int(mv[idx]), d4)] = 1.0
    out["mcts_scores"] = ms.astype(np.float32)
    return out
