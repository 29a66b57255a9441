"""The search loop of k_ladder_map (elf_amd/csrc/ladder.cuh), restated in Python over pyoracle.RefBoard's primitives: clone,
play (TryPlay2 + Play), colours, liberties and the last two moves.  The recursion of the reference (base/board.cc:299-439) is
not used here: this is the kernel's loop -- one working copy, the line's moves on a stack, a stack of open forks, reload of the
position and replay of the stack on every backtrack, the MAX_LADDER_SEARCH rule -- so that

* the loop's logic is pinned on the reference's own answers without a GPU (depth and num_call must come out equal), and
* the two quantities the kernel bounds, which the reference does not have, can be counted on any input: the plays of one
  searched point, replays included (LADDER_MAX_PLAYS), and the moves of its longest line (LADDER_STACK).

The kernel normalises the working copy's private header before every play (ply = 1, no super-ko record); a bare Board has
neither a move limit nor a super-ko test, so there is nothing to restate for that."""
import numpy as np

MAX_LADDER_SEARCH = 1024     # LADDER_MAX_SEARCH
LADDER_STACK = 1024
LADDER_MAX_PLAYS = 32000
S_OFF = 3


class Result:
    __slots__ = ("depth", "calls", "plays", "longest", "forks", "over")

    def __init__(self, depth, calls, plays, longest, forks, over):
        self.depth, self.calls, self.plays, self.longest, self.forks, self.over = depth, calls, plays, longest, forks, over

    def __repr__(self):
        return "Result(depth=%d, calls=%d, plays=%d, longest=%d, forks=%d, over=%s)" % (
            self.depth, self.calls, self.plays, self.longest, self.forks, self.over)


class Restated:
    def __init__(self, RB, max_search=MAX_LADDER_SEARCH, stack=LADDER_STACK, max_plays=LADDER_MAX_PLAYS):
        self.RB, self.n = RB, RB.n
        self.S = S = RB.n + 2
        self.max_search, self.stack, self.max_plays = max_search, stack, max_plays
        self.d4 = (-1, -S, 1, S)                                       # L, T, R, B: delta4 (base/board.h:220)
        n = RB.n
        self.coords = np.array([(y + 1) * S + (x + 1) for x in range(n) for y in range(n)])   # action a = x*n + y -> Coord

    def _view(self, b):
        """colours (the border as S_OFF) and liberties of the group on every point, indexed by Coord"""
        col, lib = self.RB.board(b)
        c = np.full(self.S * self.S, S_OFF, np.int32)
        l = np.zeros(self.S * self.S, np.int32)
        c[self.coords], l[self.coords] = col, lib
        return c, l

    def empty4(self, col, c):
        return [c + d for d in self.d4 if col[c + d] == 0]

    def candidates(self, h):
        """the kernel's prefilter on Board handle h -> actions a, ascending (the order the kernel searches them in)"""
        col, lib = self._view(h)
        info = self.RB.info(h)
        vic = int(info[1])
        ko = int(info[5]) if info[5] != 0 and info[4] == 0 and info[6] == vic else 0
        c = self.coords
        v = np.stack([col[c + d] for d in self.d4])
        l = np.stack([lib[c + d] for d in self.d4])
        nemp = (v == 0).sum(0)
        own1 = ((v == vic) & (l == 1)).sum(0)
        en3 = ((v == 3 - vic) & (l >= 3)).sum(0)
        return [int(a) for a in np.nonzero((col[c] == 0) & (c != ko) & (nemp == 2) & (own1 == 1) & (en3 == 1))[0]]

    def search(self, h, a):
        """the kernel's search of candidate action a on Board handle h (only read) -> Result"""
        RB = self.RB
        vic = int(RB.info(h)[1])
        mv = [int(self.coords[a])]        # st.mv: the line of play, mv[0] the candidate move
        forks = []                        # st.fork_at / st.fork_mv, deepest last
        ln, cnt = 1, 0
        ncall = plays = result = 0
        longest, most_forks = 1, 0
        over, reload = False, True
        wb = None
        while True:
            if plays >= self.max_plays:
                over = True
                break
            if reload:
                if wb is not None:
                    RB.free(wb)
                wb = RB.clone(h)
                cnt, reload = 0, False
            ok = RB.play(wb, mv[cnt])
            plays += 1
            if cnt + 1 < ln:              # a replay towards a fork
                if not ok:
                    over = True
                    break
                cnt += 1
                continue
            cnt += 1
            fail = False
            if not ok:
                fail = True               # TryPlay2 refused
            else:
                col, lib = self._view(wb)
                info = RB.info(wb)
                ci, mover_next = int(info[2]), int(info[1])
                assert ci == mv[cnt - 1]
                lb = int(lib[ci])
                nxt = alt = 0
                if mover_next != vic:     # the victim has just moved
                    if ln > 1:
                        if lb >= 3:
                            fail = True
                        elif lb == 2 and any(col[ci + d] == 3 - vic and lib[ci + d] == 1 for d in self.d4):
                            fail = True
                    if not fail:          # capturer's node
                        ncall += 1
                        if lb == 1:
                            result = ln
                            break
                        em = self.empty4(col, ci)
                        if lb >= 3 or len(em) <= 1:
                            fail = True
                        else:
                            e0, e1 = em[0], em[1]
                            must = 0
                            if len(self.empty4(col, e0)) == 3:
                                must = e0
                            elif len(self.empty4(col, e1)) == 3:
                                must = e1
                            if not must and ncall >= self.max_search:
                                must = e0
                            if must:
                                nxt = must
                            else:
                                nxt, alt = e0, e1
                else:                     # victim's node: the capturer has just moved
                    ncall += 1
                    if lb == 1:
                        fail = True
                    else:
                        c2 = int(info[3])
                        assert c2 == mv[cnt - 2]
                        em = self.empty4(col, c2)
                        if not em:
                            fail = True
                        else:
                            nxt = em[0]
                if not fail:
                    if ln >= self.stack:
                        over = True
                        break
                    if ln < len(mv):
                        mv[ln] = nxt
                    else:
                        mv.append(nxt)
                    if alt:
                        forks.append((ln, alt))
                        most_forks = max(most_forks, len(forks))
                    ln += 1
                    longest = max(longest, ln)
                    continue
            if not forks:
                break
            m, fm = forks.pop()
            mv[m] = fm
            ln = m + 1
            reload = True
        if wb is not None:
            RB.free(wb)
        if over:
            return Result(0, -1, plays, longest, most_forks, True)
        return Result(result, ncall, plays, longest, most_forks, False)

    def maps(self, h):
        """-> (depth int16 [NP], calls int16 [NP], list of (a, Result)): what the kernel writes for Board handle h"""
        np_ = self.n * self.n
        depth, calls = np.zeros(np_, np.int16), np.zeros(np_, np.int16)
        res = []
        for a in self.candidates(h):
            r = self.search(h, a)
            depth[a], calls[a] = r.depth, r.calls
            res.append((a, r))
        return depth, calls, res
