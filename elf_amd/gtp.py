"""GTP front-end over the device-resident engine.

Mirrors the reference's console: `GoConsoleGTP` (scripts/elfgames/go/console_lib.py:207-372) driven by `df_console.py`, i.e. the
`human_actor` batch group of GoGameSelfPlay::act (src_cpp/elfgames/go/common/game_selfplay.cc:290-330): a human move is forwarded
on the game board, `genmove` lets the MCTS AI search and play, `clear_board` finishes the game (FR_CLEAR).  Same command set,
same replies ("= ..." / "? ..."), same coordinate letters (no 'I'): protocol_version, name, version, komi, boardsize,
clear_board, play, genmove, showboard, final_score, list_commands, quit/exit.  On top of the reference's set (whose `u` / `h`
commands are commented out, console_lib.py:196-204): undo, fixed_handicap, place_free_handicap, set_free_handicap, loadsgf,
known_command -- what every GTP front-end sends -- over SelfPlay.setup / SelfPlay.undo; final_status_list and the private
elf-ownership, elf-score_estimate, elf-ladders, elf-candidates, elf-region_candidates, elf-eyes, elf-life, elf-fast_score and
elf-ld_read over the per-point answers of the board engine; lz-genmove_analyze (Leela Zero's analysing genmove, what Sabaki and
Lizzie send) and elf-analysis over the search's candidates and lines (SelfPlay.analyze).

    eng = GtpEngine(actor, board_size=19, mcts_rollout_per_thread=1600)     # actor(batch) -> dict(pi=..., V=...)
    eng.loop()                                                               # stdin/stdout, or eng.command("genmove b")
"""
import inspect
import sys

from ._lib import ElfGoError
from .engine import M_PASS, SEMI_EYE, TRUE_EYE

M_RESIGN = 1   # base/common.h:44
from .selfplay import SelfPlay


def move2xy(v):
    """console_lib.py:12-20"""
    if v.lower() == "pass":
        return -1, -1
    x = ord(v[0].lower()) - ord("a")
    if x >= 9:      # skip 'i'
        x -= 1
    y = int(v[1:]) - 1
    return x, y


def xy2move(x, y):
    """console_lib.py:23-29"""
    if x == -1 and y == -1:
        return "pass"
    if x >= 8:
        x += 1
    return chr(x + 65) + str(y + 1)


def format_analysis(n, coord, visits, winrate, prior, pv_len, pv):
    """One game's analysis (a row of each array of SelfPlay.analyze / last_analysis) as Leela-Zero-style text for an N x N board:
    one `info move <v> visits <n> winrate <w> prior <p> order <k> pv <v> <v> ...` per candidate, in rank order, joined by single
    spaces on one line.  winrate and prior are round(x * 10000); vertices are xy2move's, `pass` for M_PASS.  No `lcb` field: the
    engine has no such bound.  An analysis without candidates is the empty string."""
    S = n + 2

    def vertex(c):
        c = int(c)
        return "pass" if c == M_PASS else xy2move(c % S - 1, c // S - 1)
    out = []
    for k in range(len(coord)):
        if int(coord[k]) < 0 or int(visits[k]) <= 0:
            break
        line = [vertex(c) for c in pv[k][:int(pv_len[k])]]
        out.append("info move %s visits %d winrate %d prior %d order %d pv %s" % (
            vertex(coord[k]), int(visits[k]), int(round(float(winrate[k]) * 10000)), int(round(float(prior[k]) * 10000)), k,
            " ".join(line)))
    return " ".join(out)


# the reference's HandicapTable (base/go_state.cc:36-45) as GTP vertices, 19x19 only (it has none for 9x9)
_H4 = ("D4", "Q16", "D16", "Q4")
_H6 = _H4 + ("D10", "Q10")
_H8 = _H6 + ("K16", "K4")
HANDICAP_VERTICES = {2: ("D4", "Q16"), 3: ("D4", "Q16", "Q4"), 4: _H4, 5: _H4 + ("K10",), 6: _H6, 7: _H6 + ("K10",), 8: _H8,
                     9: _H8 + ("K10",)}


class GtpEngine:
    def __init__(self, actor, board_size=19, komi=7.5, device=0, status_playouts=256, status_seed=1, status_self_atari_thres=None,
                 ld_seed=1, ld_self_atari_thres=3, **selfplay_options):
        opts = dict(mcts_rollout_per_thread=1600, mcts_rollout_per_batch=8, mcts_puct=1.5, mcts_virtual_loss=1,
                    mcts_persistent_tree=True, policy_distri_cutoff=0, resign_thres=0.0, seed=1)
        opts.update(selfplay_options)
        self.n = int(board_size)
        self.komi = float(komi)
        self.sp = SelfPlay(board_size=self.n, num_games=1, device=device, komi=self.komi, **opts)
        self.sp.reg_callback("actor_black", actor)
        self.boards = self.sp.board_engine()
        self.exit = False
        self.status_playouts = int(status_playouts)
        self.status_seed = int(status_seed)
        # None: the status playouts fill everything but the mover's own true eyes, and no seki is reported.  A threshold t: they
        # play the reference's candidate moves (no self-atari of t stones or more), and final_status_list reports seki
        self.status_self_atari_thres = None if status_self_atari_thres is None else int(status_self_atari_thres)
        # elf-ld_read: the seed of its playouts and the candidate threshold (3: throw-ins of one or two stones stay in)
        self.ld_seed, self.ld_self_atari_thres = int(ld_seed), int(ld_self_atari_thres)
        self.commands = {k[3:]: f for k, f in inspect.getmembers(self, predicate=inspect.ismethod) if k.startswith("on_")}
        # private extensions carry the "elf-" prefix (GTP 2, section 2.13); a method name cannot hold the hyphen
        self.commands["elf-ownership"] = self.commands.pop("elf_ownership")
        self.commands["elf-score_estimate"] = self.commands.pop("elf_score_estimate")
        self.commands["elf-ladders"] = self.commands.pop("elf_ladders")
        self.commands["elf-candidates"] = self.commands.pop("elf_candidates")
        self.commands["elf-eyes"] = self.commands.pop("elf_eyes")
        self.commands["elf-life"] = self.commands.pop("elf_life")
        self.commands["elf-fast_score"] = self.commands.pop("elf_fast_score")
        self.commands["elf-region_candidates"] = self.commands.pop("elf_region_candidates")
        self.commands["elf-ld_read"] = self.commands.pop("elf_ld_read")
        self.commands["elf-analysis"] = self.commands.pop("elf_analysis")
        self.commands["lz-genmove_analyze"] = self.commands.pop("lz_genmove_analyze")
        # every finished search leaves its candidates and lines behind (elf-analysis): one small launch per move of one game
        self.analysis_moves, self.analysis_pv = 10, 16
        self.sp.set_analysis(self.analysis_moves, self.analysis_pv)
        self.info_out = None     # loop(): where lz-genmove_analyze streams its info lines while the search runs

    def close(self):
        self.boards.close()      # the ownership scratch goes before the engine it was made over
        self.sp.close()

    # ---- board queries (GoGameSelfPlay.showBoard/getNextPlayer/getLastMove/getScore, inference/Pybind.cc:31-45)
    def _info(self):
        return self.boards.info_host(n=1)

    def next_player(self):
        return "B" if int(self._info()["next_player"][0]) == 1 else "W"

    def coord2move(self, c):
        if c == M_PASS:
            return "pass"
        S = self.n + 2
        return xy2move(c % S - 1, c // S - 1)

    def move2coord(self, v):
        x, y = move2xy(v)
        if (x, y) == (-1, -1):
            return M_PASS
        if not (0 <= x < self.n and 0 <= y < self.n):
            raise ValueError("off board")
        return (y + 1) * (self.n + 2) + (x + 1)

    def showboard(self):
        col, _ = self.boards.export_board(n=1)
        col = col.cpu().numpy()[0].reshape(self.n, self.n)     # [x][y]
        letters = [xy2move(x, 0)[0] for x in range(self.n)]
        rows = ["   " + " ".join(letters)]
        for y in range(self.n - 1, -1, -1):
            rows.append("%2d " % (y + 1) + " ".join(".XO"[int(col[x, y])] for x in range(self.n)) + " %d" % (y + 1))
        rows.append("   " + " ".join(letters))
        info = self._info()
        rows.append("Next: %s  ply %d  captures B %d W %d" % (self.next_player(), int(info["ply"][0]), int(info["b_cap"][0]), int(info["w_cap"][0])))
        return "\n".join(rows)

    def check_player(self, player):
        """console_lib.py:310-322"""
        nxt = self.next_player()
        if player.lower() != nxt.lower():
            return False, "Specified next player %s is not the same as the next player %s on the board" % (player, nxt)
        return True, None

    # ---- GTP commands (console_lib.py:208-282)
    def on_protocol_version(self, items):
        return True, "2"

    def on_name(self, items):
        return True, "DF2"

    def on_version(self, items):
        return True, "1.0"

    def on_komi(self, items):
        if float(items[1]) != self.komi:
            return False, "We only support %g komi for now" % self.komi
        return True, None

    def on_boardsize(self, items):
        if items[1] != str(self.n):
            return False, "We only support %dx%d board for now" % (self.n, self.n)
        return True, None

    def _untouched(self):
        """the game has neither moved nor been set up"""
        info = self._info()
        return int(info["ply"][0]) == 1 and int(info["hist_len"][0]) == 0

    def on_clear_board(self, items):
        # M_CLEAR of the human actor (game_selfplay.cc:306-311): a game that has not started yet is left alone; one that was only
        # set up (ply still 1, its stones in the history ring) is cleared like one that has moved
        if not self._untouched():
            self.sp.restart([0])
        return True, None

    # ---- position setup and undo
    def _place(self, vertices, next_player):
        """black stones on `vertices`, `next_player` (1 / 2) to move, on a game that has not moved"""
        import numpy as np
        st = np.zeros(self.n * self.n, np.uint8)
        for v in vertices:
            x, y = move2xy(v)
            st[x * self.n + y] = 1
        self.sp.setup(st, [0], next_player)

    def _handicap(self, items):
        try:
            k = int(items[1])
        except (IndexError, ValueError):
            return False, "invalid handicap"
        if self.n != 19 or k not in HANDICAP_VERTICES:
            return False, "invalid handicap"
        if not self._untouched():
            return False, "board not empty"
        self._place(HANDICAP_VERTICES[k], 2)
        return True, " ".join(HANDICAP_VERTICES[k])

    def on_fixed_handicap(self, items):
        return self._handicap(items)

    def on_place_free_handicap(self, items):
        return self._handicap(items)

    def on_set_free_handicap(self, items):
        try:
            xy = {move2xy(v) for v in items[1:]}
        except (IndexError, ValueError):
            return False, "invalid vertex"
        if len(xy) < 2 or any(not (0 <= x < self.n and 0 <= y < self.n) for x, y in xy):
            return False, "invalid handicap"
        if not self._untouched():
            return False, "board not empty"
        self._place([xy2move(x, y) for x, y in sorted(xy)], 2)
        return True, None

    def on_undo(self, items):
        try:
            self.sp.undo(1, [0])
        except ElfGoError:
            return False, "cannot undo"
        return True, None

    def on_loadsgf(self, items):
        """loadsgf file [move_number]: the file's setup stones, then its moves up to (not including) move_number"""
        from .train import parse_sgf, sgf_setup
        if not self._untouched():
            self.sp.restart([0])
        try:
            with open(items[1], "rb") as f:
                text = f.read()
            upto = int(items[2]) - 1 if len(items) > 2 else None
            stones, k = sgf_setup(self.n, text)
            parsed = parse_sgf(self.n, text)
            if parsed is None and k == 0:
                raise ValueError("no game in the file")
            players, coords = (parsed[0], parsed[1]) if parsed is not None else ([], [])
            # to move: the colour of the first move; without moves White if there are AB stones, else Black
            first = int(players[0]) if len(players) else (2 if (stones == 1).any() else 1)
            if first not in (1, 2):
                raise ValueError("an entry without a move")
            if k or first == 2:
                self.sp.setup(stones, [0], first)
            nxt, ply = first, 1

            def play(c):
                # two passes in a row (a bridging pass next to a pass of the file) end the game and restart the board: not loadable
                nonlocal nxt, ply
                self.sp.play([c])
                nxt, ply = 3 - nxt, ply + 1
                if int(self._info()["ply"][0]) != ply:
                    raise ValueError("the game ended inside the file")
            for t, (pl, c) in enumerate(zip(players, coords)):
                if upto is not None and t >= upto:
                    break
                if int(pl) not in (1, 2):
                    raise ValueError("an entry without a move")
                if int(pl) != nxt:          # colours that do not alternate are bridged by a pass (sgf_test.cc:78-81)
                    play(M_PASS)
                play(int(c))
        except (ElfGoError, OSError, ValueError):
            if not self._untouched():
                self.sp.restart([0])
            return False, "cannot load file"
        return True, None

    def on_known_command(self, items):
        return True, "true" if len(items) > 1 and items[1] in self.commands else "false"

    def on_play(self, items):
        ret, msg = self.check_player(items[1][0])
        if not ret:
            return False, msg
        try:
            c = self.move2coord(items[2])
            self.sp.play([c])
        except Exception:
            return False, "illegal move"
        return True, None

    def on_genmove(self, items):
        ret, msg = self.check_player(items[1][0])
        if not ret:
            return False, msg
        moves = self.sp.stats()["moves"]
        while self.sp.stats()["moves"] == moves:
            self.sp.run()
        # what the search did -- not inferred from the game counter: the engine may have resigned (no move, board restarted), or
        # its move may have ended the game (two passes / move limit), in which case the board shows the next game already
        c = int(self.sp.last_moves()[0])
        if c == M_RESIGN:
            return True, "resign"
        return True, self.coord2move(c)

    # ---- search analysis: candidate moves and principal variations (SelfPlay.analyze / last_analysis)
    def _info_line(self, a):
        return format_analysis(self.n, a["coord"][0], a["visits"][0], a["winrate"][0], a["prior"][0], a["pv_len"][0], a["pv"][0])

    def on_lz_genmove_analyze(self, items):
        """lz-genmove_analyze <color> [interval_centiseconds]: genmove that reports what the search is looking at -- an info line
        whenever the interval has passed, the finished search's line at the end, then `play <vertex>` (or `play resign`).
        Without an interval only the final line is reported."""
        import time
        ret, msg = self.check_player(items[1][0])
        if not ret:
            return False, msg
        interval = float(items[2]) / 100.0 if len(items) > 2 else None
        if interval is not None and not interval >= 0:
            return False, "invalid interval"
        lines = []

        def emit(line):
            if self.info_out is not None:        # streamed: the reply opens with its first line
                self.info_out.write(("" if lines else "=\n") + line + "\n")
                self.info_out.flush()
            lines.append(line)
        moves = self.sp.stats()["moves"]
        last = time.monotonic()
        while True:
            self.sp.run()
            if self.sp.stats()["moves"] != moves:
                break
            if interval is not None and time.monotonic() - last >= interval:
                line = self._info_line(self.sp.analyze(self.analysis_moves, self.analysis_pv))
                if line:
                    emit(line)
                last = time.monotonic()
        line = self._info_line(self.sp.last_analysis())
        if line:
            emit(line)
        c = int(self.sp.last_moves()[0])
        emit("play " + ("resign" if c == M_RESIGN else self.coord2move(c)))
        return True, "\n" + "\n".join(lines)

    def on_elf_analysis(self, items):
        """The info line of the last finished search (see lz-genmove_analyze); empty before the first one."""
        return True, self._info_line(self.sp.last_analysis())

    def on_showboard(self, items):
        return True, "\n" + self.showboard()

    def on_final_score(self, items):
        if not self._untouched():             # a game that has moved or was set up: this position's score
            score = float(self.boards.evaluate(komi=self.komi, n=1).cpu()[0])     # GoGameSelfPlay::getScore
        else:
            score = float(self.sp.last_score()[0])                                # getLastScore
        return True, ("B+%.1f" % score) if score > 0 else ("W+%.1f" % -score)

    # ---- dead stones and territory by random playouts (GoEngine.ownership on game 0's current position)
    def _status_counts(self):
        """-> (stone colour per point, playouts that ended with the point black, ... white), numpy [N*N] in action order"""
        import numpy as np
        own = self.boards.ownership(np.array([self.status_seed], np.uint64), ids=[0], playouts=self.status_playouts, komi=self.komi,
                                    self_atari_thres=self.status_self_atari_thres)
        counts = own["counts"].cpu().numpy()[0]
        col = self.boards.export_board(n=1)[0].cpu().numpy()[0]
        return col, counts[0], counts[1]

    def _seki(self, col, cb, cw, dead):
        """Stones that are not dead and whose group touches an empty point that ended as neither colour's area in more than half
        of the playouts: with self-ataris kept out of the playouts, the shared liberties of a seki stay open to the end."""
        import numpy as np
        n = self.n
        g = col.reshape(n, n)
        open_pt = ((col == 0) & (2 * (self.status_playouts - cb - cw) > self.status_playouts)).reshape(n, n)
        seki = np.zeros((n, n), bool)
        seen = np.zeros((n, n), bool)
        for x0, y0 in zip(*np.nonzero(g)):
            if seen[x0, y0]:
                continue
            group, stack, touches = [], [(int(x0), int(y0))], False
            seen[x0, y0] = True
            while stack:
                x, y = stack.pop()
                group.append((x, y))
                for qx, qy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                    if not (0 <= qx < n and 0 <= qy < n):
                        continue
                    if open_pt[qx, qy]:
                        touches = True
                    elif g[qx, qy] == g[x0, y0] and not seen[qx, qy]:
                        seen[qx, qy] = True
                        stack.append((qx, qy))
            if touches:
                for x, y in group:
                    seki[x, y] = True
        return seki.reshape(-1) & ~dead

    def on_final_status_list(self, items):
        """A stone is dead iff its point ends as the opponent's area in more of the playouts than as its own colour's, else
        alive.  By default seki is not detected: `seki` is the empty list and stones in seki are reported alive (or, where the
        playouts fill their shared liberties, dead).  With status_self_atari_thres set, the playouts keep off self-ataris of that
        size, and `seki` lists the stones that are not dead and whose group touches an empty point that ended as neither colour's
        area in more than half of the playouts; `alive` then leaves them out.  A Monte-Carlo heuristic, not a proof: a dame that
        both sides happen to leave open reads the same way."""
        if len(items) < 2 or items[1] not in ("dead", "alive", "seki"):
            return False, "invalid status"
        col, cb, cw = self._status_counts()
        dead = ((col == 1) & (cw > cb)) | ((col == 2) & (cb > cw))
        seki = self._seki(col, cb, cw, dead) if self.status_self_atari_thres is not None else (col < 0)
        pick = dead if items[1] == "dead" else ((col != 0) & ~dead & ~seki) if items[1] == "alive" else seki
        return True, " ".join(xy2move(a // self.n, a % self.n) for a in range(self.n * self.n) if pick[a])

    def on_elf_ownership(self, items):
        col, cb, cw = self._status_counts()
        own = (cb - cw).reshape(self.n, self.n) / float(self.status_playouts)     # [x][y]
        return True, "\n" + "\n".join(" ".join("%5.2f" % own[x, y] for x in range(self.n)) for y in range(self.n - 1, -1, -1))

    def on_elf_score_estimate(self, items):
        col, cb, cw = self._status_counts()
        score = float(int((cb > cw).sum()) - int((cw > cb).sum())) - self.komi
        return True, ("B+%.1f" % score) if score > 0 else ("W+%.1f" % -score)

    def on_elf_ladders(self, items):
        """The points where the side to move would extend a group out of atari and still be captured in a ladder
        (GoEngine.ladder_map on game 0's current position), as VERTEX:depth pairs in board order (a = x*N + y); empty if none."""
        depth = self.boards.ladder_map(ids=[0]).cpu().numpy()[0]
        return True, " ".join("%s:%d" % (xy2move(a // self.n, a % self.n), int(depth[a])) for a in range(self.n * self.n) if depth[a])

    def on_elf_candidates(self, items):
        """elf-candidates [thres]: the reference's candidate moves of the side to move (GoEngine.candidates on game 0's current
        position; thres defaults to 1: no self-atari at all) in board order (a = x*N + y), like elf-ladders: VERTEX for a plain
        candidate, VERTEX:stones for one that is a self-atari of fewer than thres stones (stones = the size of the group the move
        would leave with one liberty); empty if there is none."""
        thres = int(items[1]) if len(items) > 1 else 1
        mask, stones = [t.cpu().numpy()[0] for t in self.boards.candidates(ids=[0], self_atari_thres=thres)]
        return True, " ".join(xy2move(a // self.n, a % self.n) + (":%d" % int(stones[a]) if stones[a] > 0 else "")
                              for a in range(self.n * self.n) if mask[a])

    # ---- static life reading (GoEngine.life_map on game 0's current position)
    def _vertex(self, a):
        return xy2move(a // self.n, a % self.n)

    def on_elf_eyes(self, items):
        """The eyes of both colours in board order (a = x*N + y), like elf-ladders: VERTEX:b / VERTEX:w for a true eye (isTrueEye),
        VERTEX:b?MOVE / VERTEX:w?MOVE for a semi-eye (isSemiEye: MOVE is the diagonal point that settles it); a point that is both
        is listed both ways; empty if there is none."""
        lm = self.boards.life_map(ids=[0])
        eye, semi = lm.eye.cpu().numpy()[0], lm.semi_move.cpu().numpy()[0]
        out = []
        for a in range(self.n * self.n):
            for c, tag in ((0, "b"), (1, "w")):
                bits = int(eye[a]) >> (4 * c)
                if bits & TRUE_EYE:
                    out.append("%s:%s" % (self._vertex(a), tag))
                if bits & SEMI_EYE:
                    out.append("%s:%s?%s" % (self._vertex(a), tag, self._vertex(int(semi[c, a]))))
        return True, " ".join(out)

    def on_elf_life(self, items):
        """The stones of the groups that live by two eyes (GivenGroupLives), in board order; a proof for the groups it lists, and
        silent about every other group."""
        alive = self.boards.life_map(ids=[0]).alive.cpu().numpy()[0]
        return True, " ".join(self._vertex(a) for a in range(self.n * self.n) if alive[a])

    def on_elf_fast_score(self, items):
        """elf-fast_score [chinese|japanese]: getFastScore from Black's side, an integer; no komi is applied, as in the reference."""
        rule = items[1] if len(items) > 1 else "chinese"
        if rule not in ("chinese", "japanese"):
            return False, "invalid rule"
        return True, "%d" % int(self.boards.fast_score(ids=[0], rule=rule).cpu()[0])

    # ---- region lists and life-and-death reading (GoEngine.region_moves / ld_read on game 0's current position)
    def _box(self, v1, v2):
        """two vertices, opposite corners -> the half-open box (left, top, right, bottom) that holds both"""
        (x1, y1), (x2, y2) = move2xy(v1), move2xy(v2)
        if not all(0 <= v < self.n for v in (x1, y1, x2, y2)):
            raise ValueError("off board")
        return (min(x1, x2), min(y1, y2), max(x1, x2) + 1, max(y1, y2) + 1)

    def on_elf_region_candidates(self, items):
        """elf-region_candidates VERTEX VERTEX [thres]: elf-candidates inside the box whose opposite corners the two vertices are
        (FindAllCandidateMovesInRegion), in elf-candidates' format; thres defaults to 1."""
        if len(items) < 3:
            return False, "two vertices expected"
        try:
            box = self._box(items[1], items[2])
            thres = int(items[3]) if len(items) > 3 else 1
        except (IndexError, ValueError):
            return False, "invalid vertex"
        mask = self.boards.region_moves(ids=[0], regions=[box], self_atari_thres=thres)[0].cpu().numpy()[0]
        stones = self.boards.candidates(ids=[0], self_atari_thres=thres)[1].cpu().numpy()[0]
        return True, " ".join(self._vertex(a) + (":%d" % int(stones[a]) if stones[a] > 0 else "")
                              for a in range(self.n * self.n) if mask[a])

    def on_elf_ld_read(self, items):
        """elf-ld_read [VERTEX VERTEX] [playouts]: life-and-death reading of the box whose opposite corners the two vertices are
        (none: the bounding box of the stones) by region playouts.  First line: `attacker b|w defender b|w to_move b|w lives a/b
        survives a/b best VERTEX|pass|none` (a of b playouts ended with a living defender group in the box / a defender stone in
        the box); then one line `VERTEX playouts lived survived` per first move, in board order, `pass` last.  Seed and threshold
        are the constructor's ld_seed and ld_self_atari_thres: the same position gives the same reply."""
        import numpy as np
        args = items[1:]
        box = None
        try:
            if len(args) >= 2 and not args[0].isdigit():
                box = self._box(args[0], args[1])
                args = args[2:]
            playouts = int(args[0]) if args else self.status_playouts
        except (IndexError, ValueError):
            return False, "invalid arguments"
        if playouts <= 0 or len(args) > 1:
            return False, "invalid arguments"
        rd = self.boards.ld_read(np.array([self.ld_seed], np.uint64), ids=[0], regions=None if box is None else [box],
                                 playouts=playouts, self_atari_thres=self.ld_self_atari_thres)
        info, stats, first = rd.info.cpu().numpy()[0], rd.stats.cpu().numpy()[0], rd.first.cpu().numpy()[0]
        NP = self.n * self.n
        name = lambda a: "pass" if a == NP else self._vertex(a)
        best = rd.best_move()[0]
        lines = ["attacker %s defender %s to_move %s lives %d/%d survives %d/%d best %s" % (
            " bw"[int(info[4])], " bw"[int(info[5])], " bw"[int(info[6])], int(stats[0]), playouts, int(stats[1]), playouts,
            "none" if best is None else name(best))]
        lines += ["%s %d %d %d" % (name(a), int(first[0, a]), int(first[1, a]), int(first[2, a])) for a in range(NP + 1) if first[0, a]]
        return True, "\n".join(lines)

    def on_list_commands(self, items):
        return True, "\n".join(self.commands.keys())

    def on_quit(self, items):
        self.exit = True
        return True, None

    def on_exit(self, items):
        return self.on_quit(items)

    # ---- protocol
    def command(self, line):
        """One GTP command line -> the reply text ("= ..." or "? ..."), console_lib.py:324-372"""
        items = line.split()
        if not items:
            return "? Invalid input\n\n"
        try:
            ret, msg = self.commands[items[0]](items)
        except KeyError:
            return "? unknown command\n\n"
        except Exception as e:
            return "? Invalid command (%s)\n\n" % e
        return "%s %s\n\n" % ("=" if ret else "?", msg if msg is not None else "")

    def loop(self, fin=sys.stdin, fout=sys.stdout):
        for line in fin:
            # lz-genmove_analyze writes its reply line by line while the search runs; what is left to write is the blank line
            self.info_out = fout if line.split()[:1] == ["lz-genmove_analyze"] else None
            reply = self.command(line.strip())
            fout.write("\n" if self.info_out is not None and reply.startswith("= \n") else reply)
            self.info_out = None
            fout.flush()
            if self.exit:
                break
