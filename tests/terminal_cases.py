"""Crafted positions for the rules of the game (utils.py:199-235 is_game_over) over the whole range af_engine_create accepts:
board_size 2..16, goal 2..board_size.  Shared by tests/golden/make_rules_envelope.py (which records the unmodified reference's
answers), tests/test_rules_envelope.py (CPU) and tests/test_gpu_terminal_envelope.py (the engine's three device forms of the rule).

Deterministic: every random choice comes from a RandomState seeded by (S, goal).  Boards are int8[S][S] seen from the side to move
(+1 mine, -1 theirs, utils.py:185); cell c = i * S + j.

cases(S, goal)  -> list of Case: `child` is the position after the mover has placed the stone at `last` (so child[last] == -1); the
                   position before, root_of(case) = -child with `last` cleared, is terminal for neither colour.
roots(S, goal)  -> list of Root: positions handed over as they are (no last move), decided and undecided, for the two-sided scan.
thin(items, cap)-> the deterministic, stratified choice that caps a list: round-robin over the strata (class, direction, position of
                   `last`, step, tag), so no class and no direction is emptied; the `cells` class is never thinned.
"""
import collections

import numpy as np

import oracle

PAIRS = [(2, 2), (3, 2), (4, 4), (5, 5), (6, 6), (7, 7), (8, 5), (8, 8), (9, 6), (10, 8), (10, 10), (11, 7), (11, 8), (11, 9),
         (11, 11), (12, 5), (12, 8), (13, 9), (13, 13), (14, 8), (15, 8), (16, 5), (16, 8), (16, 9), (16, 16)]
CLASSES = ("line", "short", "over", "wrap", "word", "cells", "draw", "clutter")
DIRS = ((1, 0), (0, 1), (1, 1), (-1, 1))            # down, right, down-right, up-right: the scan order of utils.py:210-232
DIR_NAMES = ("down", "right", "down-right", "up-right")
POS_NAMES = ("first", "middle", "final")
WORD_EDGES = (64, 128, 192)                         # cells 63/64, 127/128, 191/192: the 64-bit words of a bitboard
ROOT_KINDS = ("mine", "theirs", "both", "short", "wrap", "draw")
CAP = 512

# dir / pos / step are -1 where they do not apply; tag tells strata of one class apart (a border, a word edge, the source class)
Case = collections.namedtuple("Case", "child last cls dir pos step tag")
Root = collections.namedtuple("Root", "board kind tag")


def root_of(case):
    r = (-case.child).astype(np.int8)
    r.reshape(-1)[case.last] = 0
    return r


def _terminal(board, goal):
    return oracle.is_game_over(board, goal)[0]


def _runs(S, length, d):
    """Every run of `length` cells along direction d that lies on the board: lists of cells, in order of their first cell."""
    di, dj = DIRS[d]
    out = []
    for i0 in range(S):
        for j0 in range(S):
            i1, j1 = i0 + di * (length - 1), j0 + dj * (length - 1)
            if 0 <= i1 < S and 0 <= j1 < S:
                out.append([(i0 + di * k) * S + (j0 + dj * k) for k in range(length)])
    return out


def _touch(run, S):
    """Borders and corners a run touches."""
    rows, cols = [c // S for c in run], [c % S for c in run]
    t = set()
    if 0 in rows:
        t.add("top")
    if S - 1 in rows:
        t.add("bottom")
    if 0 in cols:
        t.add("left")
    if S - 1 in cols:
        t.add("right")
    for name, c in (("c00", 0), ("c0S", S - 1), ("cS0", S * (S - 1)), ("cSS", S * S - 1)):
        if c in run:
            t.add(name)
    return t


def _picked_runs(S, length, d, rng, interior=2):
    """(run, tag): for every corner the direction can reach a run that holds it, for every border one that touches it (the middle
    one of those that do), then a few that touch nothing."""
    runs = _runs(S, length, d)
    out, seen = [], set()

    def take(run, tag):
        if run[0] not in seen:
            seen.add(run[0])
            out.append((run, tag))

    for name in ("c00", "c0S", "cS0", "cSS", "top", "bottom", "left", "right"):
        hit = [r for r in runs if name in _touch(r, S)]
        if hit:
            take(hit[0] if name[0] == "c" else hit[len(hit) // 2], name)
    inner = [r for r in runs if not _touch(r, S)]
    for k in rng.permutation(len(inner))[:interior]:
        take(inner[int(k)], "inner")
    return out


def _board(S, cells, colour=-1):
    b = np.zeros((S, S), np.int8)
    b.reshape(-1)[list(cells)] = colour
    return b


def _straddles(run, edge):
    """Index k such that run[k] and run[k + 1] lie on the two sides of a word edge, or -1."""
    for k in range(len(run) - 1):
        lo, hi = min(run[k], run[k + 1]), max(run[k], run[k + 1])
        if lo < edge <= hi:
            return k
    return -1


def _stripe(S):
    return np.fromfunction(lambda i, j: ((i // 2 + j) % 2) * 2 - 1, (S, S)).astype(np.int8)


def _all_cases(S, goal):
    rng = np.random.RandomState(1000 * S + goal)
    C = S * S
    out = []

    def add(child, last, cls, d=-1, pos=-1, step=-1, tag=""):
        child = np.ascontiguousarray(child, np.int8)
        assert child.reshape(-1)[last] == -1
        c = Case(child, int(last), cls, d, pos, step, tag)
        if _terminal(root_of(c), goal):
            return False
        out.append(c)
        return True

    # line: exactly `goal` in a row, `last` at the first, a middle and the final stone
    for d in range(4):
        for run, tag in _picked_runs(S, goal, d, rng):
            for pos, k in enumerate((0, goal // 2, goal - 1)):
                add(_board(S, run), run[k], "line", d, pos, tag=tag)
    # short: goal - 1 in a row
    if goal >= 2:
        for d in range(4):
            for n, (run, tag) in enumerate(_picked_runs(S, goal - 1, d, rng)):
                add(_board(S, run), run[(0, (goal - 1) // 2, goal - 2)[n % 3]], "short", d, n % 3, tag=tag)
    # over: goal + 1 in a row; the last stone joins two runs that are both shorter than goal
    if goal + 1 <= S:
        for d in range(4):
            for n, (run, tag) in enumerate(_picked_runs(S, goal + 1, d, rng)):
                add(_board(S, run), run[1 + n % (goal - 1)], "over", d, 1, tag=tag)
    found_step1 = False
    # wrap: consecutive in flat index space with step 1, S + 1 or S - 1, but not along a line of the board
    for step in (1, S + 1, S - 1):
        if step == 1 and S == 2 and found_step1:          # (on a 2x2 board S - 1 is the step 1 again)
            continue
        found_step1 = True
        for length in (goal, goal + 1):
            found = []
            for c in range(C):
                cells = [c + k * step for k in range(length)]
                if cells[-1] >= C:
                    break
                x0 = c % S
                leaves = (x0 + length - 1 >= S) if step in (1, S + 1) else (x0 - (length - 1) < 0)
                if leaves and len(set(cells)) == length:
                    found.append(cells)
            keep = {0, len(found) // 2, len(found) - 1} | {int(k) for k in rng.permutation(len(found))[:3]}
            keep |= {n for n, cells in enumerate(found) if any(_straddles(cells, e) >= 0 for e in WORD_EDGES) and n % 3 == 0}
            for m, n in enumerate(sorted(k for k in keep if 0 <= k < len(found))):
                cells = found[n]
                # the last stone may not leave a run of goal behind it: a stone inside the sequence
                order = [(m + q) % length for q in range(length)]
                for k in order:
                    if add(_board(S, cells), cells[k], "wrap", step=step, tag="len%+d" % (length - goal)):
                        break
    # word: line and short runs that straddle a word edge of the bitboard, `last` on either side of it
    for edge in WORD_EDGES:
        if C <= edge:
            continue
        for length in (goal, goal - 1):
            if length < 2:
                continue
            for d in range(4):
                hit = [(r, _straddles(r, edge)) for r in _runs(S, length, d)]
                hit = [(r, k) for r, k in hit if k >= 0]
                for r, k in hit[len(hit) // 2:len(hit) // 2 + 1]:
                    for kk in (k, k + 1):
                        add(_board(S, r), r[kk], "word", d, -1, tag="%d%s" % (edge, "line" if length == goal else "short"))
    # cells: every cell of the board is `last` once, in a short run through it
    for c in range(C):
        done = False
        for q in range(4):
            d = (c + q) % 4
            di, dj = DIRS[d]
            n = max(goal - 1, 1)
            for k0 in range(n):
                k = (c + k0) % n
                i0, j0 = c // S - di * k, c % S - dj * k
                i1, j1 = i0 + di * (n - 1), j0 + dj * (n - 1)
                if min(i0, j0, i1, j1) >= 0 and max(i0, j0, i1, j1) < S:
                    run = [(i0 + di * t) * S + (j0 + dj * t) for t in range(n)]
                    done = add(_board(S, run), c, "cells", d)
                    break
            if done:
                break
        assert done, (S, goal, c)
    # draw: the full board without a run longer than 2, and the same board with one line that the last stone completes
    if goal >= 3:
        stripe = _stripe(S)
        theirs = [int(c) for c in np.flatnonzero(stripe.reshape(-1) == -1)]
        for c in sorted({theirs[0], theirs[len(theirs) // 2], theirs[-1]}):
            add(stripe, c, "draw", tag="drawn")
        won = 0
        for d in (1, 0, 2, 3):
            runs = _runs(S, goal, d)
            for n in rng.permutation(len(runs)):
                run = runs[int(n)]
                b = stripe.copy()
                b.reshape(-1)[run] = -1
                for k in rng.permutation(goal):
                    c = Case(b, run[int(k)], "draw", d, -1, -1, "won")
                    if not _terminal(root_of(c), goal) and oracle.is_game_over(b, goal) == (True, -1.0):
                        out.append(c)
                        won += 1
                        break
                else:
                    continue
                break
        assert won or S < 3
    # clutter: copies of line, short and wrap cases with random stones of both colours on the other cells
    src = [c for c in out if c.cls in ("line", "short", "wrap")]
    for n, c in enumerate(src):
        if n % 4:
            continue
        fill = 0.1 + 0.5 * rng.rand()
        noise = rng.choice([-1, 0, 1], size=(S, S), p=[fill / 2, 1 - fill, fill / 2]).astype(np.int8)
        b = np.where(c.child != 0, c.child, noise).astype(np.int8)
        add(b, c.last, "clutter", c.dir, c.pos, c.step, tag=c.cls)
    return out


def _stratum(x):
    if not isinstance(x, Case):
        return (x.kind, x.tag)
    return (x.cls, x.dir, x.pos, x.step, x.tag if x.cls in ("wrap", "word", "draw", "clutter") else "")


def thin(items, cap=CAP):
    """At most `cap` items: everything of the `cells` class, then one item of every stratum in turn until the cap is reached.
    The order of the survivors is the order of `items`."""
    if len(items) <= cap:
        return list(items)
    keep = [n for n, x in enumerate(items) if isinstance(x, Case) and x.cls == "cells"]
    strata = collections.OrderedDict()
    for n, x in enumerate(items):
        if not (isinstance(x, Case) and x.cls == "cells"):
            strata.setdefault(_stratum(x), []).append(n)
    assert len(keep) + len(strata) <= cap, "the cap would empty a stratum"
    depth = 0
    while len(keep) < cap:
        took = False
        for members in strata.values():
            if depth < len(members) and len(keep) < cap:
                keep.append(members[depth])
                took = True
        if not took:
            break
        depth += 1
    return [items[n] for n in sorted(keep)]


_cache = {}


def cases(S, goal, cap=CAP):
    """The crafted cases of a pair, thinned to `cap`.  The C oracle's rule function classifies; tests/golden/rules_envelope.npz pins
    it, the host mirror and the unmodified reference to one another on exactly these boards."""
    key = (S, goal, cap)
    if key not in _cache:
        _cache[key] = thin(_all_cases(S, goal), cap)
    return _cache[key]


def roots(S, goal):
    """Positions for the two-sided scan of a root: a line of the side to move only, of the opponent only, of both (rows or columns
    swapped, so that the cell-major scan order of utils.py:208-232 decides), and the short, wrap and draw boards in both colours."""
    key = (S, goal, "roots")
    if key in _cache:
        return _cache[key]
    rng = np.random.RandomState(5000 + 1000 * S + goal)
    out = []
    for kind, colour in (("mine", 1), ("theirs", -1)):
        for d in range(4):
            runs = _runs(S, goal, d)
            pick = {0, len(runs) // 2, len(runs) - 1}
            for e in WORD_EDGES:
                pick |= set([n for n, r in enumerate(runs) if _straddles(r, e) >= 0][:1])
            for n in sorted(pick):
                b = _board(S, runs[n], colour)
                for c in rng.permutation(S * S)[:goal - 1]:          # a few scattered stones of the other colour: no line
                    if b.reshape(-1)[c] == 0:
                        b.reshape(-1)[c] = -colour
                assert oracle.is_game_over(b, goal) == (True, float(colour))
                out.append(Root(b, kind, DIR_NAMES[d]))
    both = np.zeros((S, S), np.int8)
    both[0, :goal], both[1, :goal] = -1, 1
    for b, tag in ((both, "rows"), (-both, "rows-"), (both.T, "cols"), (-both.T, "cols-")):
        out.append(Root(np.ascontiguousarray(b, np.int8), "both", tag))
    for c in cases(S, goal):
        if c.cls in ("wrap", "draw") or (c.cls == "short" and c.pos == 0):
            out.append(Root(c.child, c.cls, "theirs"))
            out.append(Root(np.ascontiguousarray(-c.child, np.int8), c.cls, "mine"))
    _cache[key] = out
    return out


def state_of(board):
    """The state string (utils.py:156-175) for a failure message."""
    return oracle.board_to_state(board)


def describe(case):
    d = DIR_NAMES[case.dir] if case.dir >= 0 else "-"
    p = POS_NAMES[case.pos] if case.pos >= 0 else "-"
    return "class %s dir %s last %d (%s) step %d tag %s state %s" % (case.cls, d, case.last, p, case.step, case.tag,
                                                                       state_of(case.child))
