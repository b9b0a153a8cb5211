"""Generators, numpy statements and comparisons for the device replay ring (csrc/af_replay.hip, alphafive_amd/replay.py), in plain
numpy.  tests/test_replay_reference_cpu.py checks every condition stated here and that every comparison rejects the planted faults,
without a GPU; tests/test_gpu_replay_exact.py holds the kernels to the statements bit for bit.

THE AUGMENTATION (augment_reference).  The three input planes (mine = board == 1, theirs = board == -1, a one-hot plane of the last
move, all zero for none) and the policy are turned by np.rot90(., k) and then, if `flip`, mirrored by np.flip(axis 0).  No table for
the last move: its plane turns with the board.  tests/golden/replay_symmetries.npz records that this is what the unmodified
reference's RandomStack.get_data (utils.py:118-146) returns; scripted_draws() is how its three draws are dictated.

THE GATHER (sample_cases, sample_triples, sample_expected, sample_model).  Per board size C + 1 positions, position p < C with last
move p and position C with none, each on a board whose 8 images are pairwise distinct, policy[p][c] = p C + c (exact in fp32: at most
65,791), value and weight distinct per position; all 8 (C + 1) (position, k, flip) triples in one fixed shuffled order.  sample_model
restates the kernel's index arithmetic (the inverse map of the board, the forward map of the last move, slot = (head + index) mod
capacity) over a RingMirror and takes the planted faults.

THE PACKED APPEND (packed_episodes, packed_buffer, packed_expected, packed_model).  Hand-off buffers in the layout of
include/af_engine.h af_engine_pack_episodes, built here word by word; what the ring must hold afterwards is
engine.unpack_episodes + engine.assemble_episode on the same array (tests/test_host_utils.py pins those to the reference's records);
packed_model restates the kernel's decode and takes the planted faults.

All comparisons are on bits (float arrays through their uint32 views): nothing here rounds.
"""
import contextlib
import functools
import random

import numpy as np

SIZES = tuple(range(3, 17))                      # every board size af_replay_create accepts
PACKED_SIZES = (3, 8, 11, 12, 15, 16)            # smallest; 64 cells = one full 64-bit word; standard; the first size with four key
                                                 # words per colour (144 cells); the closed-loop board; every bit of all four words
SYMMETRIES = tuple((k, f) for f in (0, 1) for k in range(4))
GAMMA = 0.94
SAMPLE_FAULTS = ("k_inverse", "flip_first", "last_unturned", "last_inverse", "horizontal_flip", "no_head")
PACKED_FAULTS = ("colours_swapped", "word_xor_1", "halves_swapped", "value_sign", "weight_row", "last_of_next_ply")


# ---------------------------------------------------------------------------------------------------------------------------
# the augmentation
# ---------------------------------------------------------------------------------------------------------------------------
def images(a):
    """the 8 images of a square array, in SYMMETRIES order"""
    return [np.flip(np.rot90(a, k), axis=0) if f else np.rot90(a, k) for k, f in SYMMETRIES]


def images_distinct(board):
    return len(set(np.ascontiguousarray(im).tobytes() for im in images(board))) == 8


def augment_reference(board, policy, last, k, flip):
    """(board int[S,S] or [C], policy float[C] or [S,S], last = cell index, or -1 / None for none, k quarter turns, flip)
    -> (planes float32[3,S,S], policy float32[C])."""
    board = np.asarray(board)
    S = int(round(np.sqrt(board.size)))
    board = board.reshape(S, S)
    planes = np.zeros((3, S, S), np.float32)
    planes[0] = board == 1
    planes[1] = board == -1
    if last is not None and int(last) >= 0:
        planes[2].reshape(-1)[int(last)] = 1
    pol = np.asarray(policy, np.float32).reshape(S, S)
    planes = np.rot90(planes, int(k), axes=(1, 2))
    pol = np.rot90(pol, int(k))
    if flip:
        planes = np.flip(planes, axis=1)
        pol = np.flip(pol, axis=0)
    return np.ascontiguousarray(planes), np.ascontiguousarray(pol).reshape(S * S)


@contextlib.contextmanager
def scripted_draws(idx, turns, flips):
    """Dictates the three draws of RandomStack.get_data (utils.py:120, 129, 136) in the calling process: np.random.choice with a
    size returns `idx`, without one the next entry of `turns`; random.choice returns 1 (flip) or 2 by the next entry of `flips`.
    Both are put back on the way out, and the script must have been used up."""
    tq, fq = [int(k) for k in turns], [int(f) for f in flips]

    def np_choice(a, size=None, replace=True, p=None):
        if size is not None:
            assert size == len(idx) and not replace
            return np.asarray(idx, np.int64)
        return np.int64(tq.pop(0))

    def py_choice(seq):
        assert list(seq) == [1, 2]
        return 1 if fq.pop(0) else 2

    saved = np.random.choice, random.choice
    np.random.choice, random.choice = np_choice, py_choice
    try:
        yield
    finally:
        np.random.choice, random.choice = saved
    assert not tq and not fq


def scripted_get_data(stack, idx, turns, flips):
    """get_data of a host RandomStack (the project's or the reference's) on dictated draws, in calls of at most len(stack.data)
    samples (get_data never returns more than the stack holds) -> its four arrays, concatenated"""
    step, parts = len(stack.data), []
    for lo in range(0, len(idx), step):
        with scripted_draws(idx[lo:lo + step], turns[lo:lo + step], flips[lo:lo + step]):
            parts.append(stack.get_data(len(idx[lo:lo + step])))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def host_records(board_to_state, boards, policies, last, values, weights):
    """positions as the 5-tuples RandomStack keeps (state string, policy[S,S], (i, j) or None, value, weight)"""
    S = int(round(np.sqrt(boards.shape[1])))
    return [(board_to_state(b.reshape(S, S)), p.reshape(S, S).copy(), None if la < 0 else (int(la) // S, int(la) % S), float(v),
             np.float32(w)) for b, p, la, v, w in zip(boards, policies, last, values, weights)]


def fixture_position(S):
    """the one position per size tests/golden/replay_symmetries.npz records: a board whose 8 images are pairwise distinct,
    policy = arange(C), last move at cell 1 -> (board int8[S,S], policy float32[C], 1)"""
    rng = np.random.RandomState(4000 + S)
    while True:
        board = rng.randint(-1, 2, (S, S)).astype(np.int8)
        if images_distinct(board):
            return board, np.arange(S * S, dtype=np.float32), 1


# ---------------------------------------------------------------------------------------------------------------------------
# a ring on the host: what every physical slot of an af_replay handle holds
# ---------------------------------------------------------------------------------------------------------------------------
FIELDS = ("boards", "policies", "last", "values", "weights")


def junk_positions(S, n, seed):
    """n arbitrary positions as af_replay_append takes them (boards, policies, last, values, weights)"""
    rng = np.random.RandomState(seed)
    C = S * S
    return (rng.randint(-1, 2, (n, C)).astype(np.int8), rng.rand(n, C).astype(np.float32) + 100.0,
            rng.randint(-1, C, n).astype(np.int32), rng.randn(n).astype(np.float32) - 50.0, rng.rand(n).astype(np.float32) + 7.0)


class RingMirror(object):
    """Physical slots, head and count of a ring of `cap` positions, moved as include/af_replay.h says the calls move them."""

    def __init__(self, S, cap):
        C = S * S
        self.S, self.C, self.cap, self.head, self.count = S, C, cap, 0, 0
        self.boards = np.zeros((cap, C), np.int8)
        self.policies = np.zeros((cap, C), np.float32)
        self.last = np.zeros(cap, np.int32)
        self.values = np.zeros(cap, np.float32)
        self.weights = np.zeros(cap, np.float32)
        self.written = np.zeros(cap, bool)

    def slots(self, first, n):
        return (self.head + first + np.arange(n)) % self.cap

    def append(self, boards, policies, last, values, weights):
        n = len(last)
        assert self.count + n <= self.cap
        s = self.slots(self.count, n)
        self.boards[s], self.last[s], self.values[s], self.weights[s] = boards, last, values, weights
        self.policies[s] = np.asarray(policies, np.float32).reshape(n, self.C)
        self.written[s] = True
        self.count += n

    def skip(self, n):
        """an append that moved the count and wrote nothing"""
        assert self.count + n <= self.cap
        self.count += n

    def drop(self, n):
        assert 0 <= n <= self.count
        self.head = (self.head + n) % self.cap
        self.count -= n

    def logical(self, first=0, n=None):
        """positions first .. first + n - 1 counted from the oldest, in order -> the five arrays"""
        n = self.count - first if n is None else n
        s = self.slots(first, n)
        assert self.written[s].all()
        return tuple(getattr(self, f)[s] for f in FIELDS)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def differing(got, want, names):
    """names of the arrays of `got` that do not equal `want`'s in shape, type or bits, each with its first differing flat index"""
    out = []
    for g, w, name in zip(got, want, names):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            out.append("%s: %s %s for %s %s" % (name, g.dtype, g.shape, w.dtype, w.shape))
            continue
        bad = np.flatnonzero(bits(g).reshape(-1) != bits(w).reshape(-1))
        if len(bad):
            out.append("%s: %d of %d elements differ, first at flat index %d (%r for %r)" %
                       (name, len(bad), g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the gather kernel's cases
# ---------------------------------------------------------------------------------------------------------------------------
SAMPLE_OUTPUTS = ("boards", "weights", "values", "policies")


@functools.lru_cache(maxsize=None)
def sample_cases(S):
    """-> (boards int8[C+1,C], policies float32[C+1,C], last int32[C+1], values float32[C+1], weights float32[C+1], redraws)"""
    C = S * S
    rng = np.random.RandomState(1000 + S)
    boards, redraws = [], 0
    for _ in range(C + 1):
        while True:
            b = rng.randint(-1, 2, (S, S)).astype(np.int8)
            if images_distinct(b):
                break
            redraws += 1
        boards.append(b.reshape(C))
    p = np.arange(C + 1)
    policies = (p[:, None] * C + np.arange(C)[None, :]).astype(np.float32)
    last = np.append(np.arange(C), -1).astype(np.int32)
    values = (np.where(p % 2 == 0, 1.0, -1.0) * (p + 1) / 512.0).astype(np.float32)          # multiples of 2^-9: exact
    weights = (1.0 + p / 1024.0).astype(np.float32)
    out = (np.stack(boards), policies, last, values, weights)
    for a in out:
        a.setflags(write=False)
    return out + (redraws,)


@functools.lru_cache(maxsize=None)
def sample_triples(S):
    """every (position, k, flip) once, 8 (C + 1) of them, in a fixed shuffled order -> three int32 arrays"""
    C = S * S
    t = np.array([(p, k, f) for p in range(C + 1) for k, f in SYMMETRIES], np.int32)
    t = t[np.random.RandomState(2000 + S).permutation(len(t))]
    out = tuple(np.ascontiguousarray(t[:, i]) for i in range(3))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sample_expected(S):
    """augment_reference on every triple of sample_triples(S) -> boards[N,3,S,S], weights[N], values[N], policies[N,C], float32"""
    boards, policies, last, values, weights, _ = sample_cases(S)
    idx, turns, flip = sample_triples(S)
    aug = [augment_reference(boards[p], policies[p], last[p], k, f) for p, k, f in zip(idx, turns, flip)]
    out = (np.stack([a[0] for a in aug]), weights[idx].copy(), values[idx].copy(), np.stack([a[1] for a in aug]))
    for a in out:
        a.setflags(write=False)
    return out


def sample_ring(S, pad=5):
    """A RingMirror of C + 1 + pad slots holding sample_cases(S) across its end: every slot is written with junk and dropped
    (so all of them hold known bytes and head has moved), junk moves the head on to half the cases before the end, then the
    cases go in.  -> (mirror, the appends and drops that build it, in order: ("append", five arrays) / ("drop", n))"""
    C = S * S
    n = C + 1
    cap = n + pad
    ring, ops = RingMirror(S, cap), []

    def do(kind, arg):
        ops.append((kind, arg))
        ring.append(*arg) if kind == "append" else ring.drop(arg)

    do("append", junk_positions(S, cap, 5000 + S))
    do("drop", cap)
    move = cap - n // 2                              # the head this leaves is the slot of case 0
    do("append", junk_positions(S, move, 6000 + S))
    do("drop", move)
    do("append", sample_cases(S)[:5])
    assert ring.head == cap - n // 2 and ring.count == n
    return ring, ops


def _turn(i, j, S):
    """one np.rot90 turn sends cell (i, j) to (S-1-j, i)"""
    return S - 1 - j, i


def _unturn(i, j, S):
    return j, S - 1 - i


def sample_model(ring, idx, turns, flip, fault=None):
    """af_replay_sample_kernel's arithmetic over a RingMirror: per sample the physical slot (head + index) mod capacity, per output
    cell the source cell (undo the flip, then undo k turns), the last move by the forward map (k turns, then the flip).
    `fault`: one of SAMPLE_FAULTS.  -> the four outputs as sample_expected gives them."""
    S, C = ring.S, ring.C
    N = len(idx)
    ob, op = np.zeros((N, 3, C), np.float32), np.zeros((N, C), np.float32)
    ow, ov = np.zeros(N, np.float32), np.zeros(N, np.float32)
    oi, oj = np.divmod(np.arange(C), S)
    for b in range(N):
        slot = int(idx[b]) if fault == "no_head" else (ring.head + int(idx[b])) % ring.cap
        k, f = int(turns[b]), int(flip[b])
        if fault == "k_inverse":
            k = (4 - k) % 4
        si, sj = oi.copy(), oj.copy()
        if fault == "flip_first":                    # out = rot90(flip(x)): undo the turns, then the flip
            for _ in range(k):
                si, sj = _unturn(si, sj, S)
            if f:
                si = S - 1 - si
        else:
            if f and fault == "horizontal_flip":
                sj = S - 1 - sj
            elif f:
                si = S - 1 - si
            for _ in range(k):
                si, sj = _unturn(si, sj, S)
        src = si * S + sj
        la = int(ring.last[slot])
        if la >= 0 and fault != "last_unturned":
            i, j = divmod(la, S)
            if fault == "flip_first" and f:
                i = S - 1 - i
            for _ in range(k):
                i, j = _unturn(i, j, S) if fault == "last_inverse" else _turn(i, j, S)
            if f and fault == "horizontal_flip":
                j = S - 1 - j
            elif f and fault != "flip_first":
                i = S - 1 - i
            la = i * S + j
        v = ring.boards[slot][src]
        ob[b, 0], ob[b, 1] = v == 1, v == -1
        if la >= 0:
            ob[b, 2, la] = 1
        op[b] = ring.policies[slot][src]
        ow[b], ov[b] = ring.weights[slot], ring.values[slot]
    return ob.reshape(N, 3, S, S), ow, ov, op


# ---------------------------------------------------------------------------------------------------------------------------
# packed hand-off buffers
# ---------------------------------------------------------------------------------------------------------------------------
def key_words(S):
    """64-bit words of a position key: two bitboards (mine, theirs) of 2 words up to 128 cells, of 4 above"""
    return 4 if S * S <= 128 else 8


def packed_lengths(S):
    """T = 1, T = 2, one odd and one even length in between, T = C (the longest an episode gets: the last row of the weight table)"""
    C = S * S
    return (1, 2, 5, 4, C) if C <= 9 else (1, 2, 7, 10, C)


ARBITRARY_FINAL = 0x3EB7C9A5                       # 0.35896..., a final value no game produces: its bits must pass through
FINALS = (0x3F800000, 0xBF800000, 0x00000000, ARBITRARY_FINAL, 0x00000000)       # +1, -1, a draw, arbitrary, a draw (the full board)
SPECIAL_POLICY_BITS = (0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000)


@functools.lru_cache(maxsize=None)
def packed_episodes(S):
    """The five episodes of one buffer.  Ply t of an episode holds the first t cells of the episode's permutation of the cells,
    stone j being the mover's own ("mine") where t - j is even: colours alternate with the side to move.  The last cell of the
    longest episode's permutation never gets a stone there and the one before it only the opponent's, so the two middle episodes
    start with those two.  Policies are arbitrary
    finite bit patterns (no NaN, no infinity) with -0.0, +0.0, subnormals and the largest finite values planted among them."""
    C, K = S * S, key_words(S)
    KW = K // 2
    rng = np.random.RandomState(3000 + S)
    lengths = packed_lengths(S)
    perms = [rng.permutation(C) for _ in lengths]
    for e in (2, 3):
        tail = perms[4][[C - 1, C - 2]]
        perms[e] = np.concatenate([tail, perms[e][~np.isin(perms[e], tail)]])
    eps, planted = [], 0
    for e, T in enumerate(lengths):
        perm = perms[e]
        keys = np.zeros((T, K), np.uint64)
        for t in range(T):
            for j in range(t):
                c = int(perm[j])
                w = c // 64 + (0 if (t - j) % 2 == 0 else KW)
                keys[t, w] |= np.uint64(1) << np.uint64(c % 64)
        pol = rng.randint(0, 2 ** 32, size=(T, C), dtype=np.uint64).astype(np.uint32)
        pol[((pol >> np.uint32(23)) & np.uint32(0xFF)) == 0xFF] ^= np.uint32(0x40000000)      # exponent 0xFF -> 0xBF: finite
        for t in range(T):                           # min(8, C // 3) of the special patterns per ply, taken in rotation
            cells = rng.permutation(C)[:min(len(SPECIAL_POLICY_BITS), C // 3)]
            pol[t, cells] = [SPECIAL_POLICY_BITS[(planted + i) % len(SPECIAL_POLICY_BITS)] for i in range(len(cells))]
            planted += len(cells)
        eps.append(dict(game=10 + 3 * e, seq=e % 2, T=T, final_bits=FINALS[e], keys=keys, policy_bits=pol,
                        visits=rng.randint(0, 500, size=(T, C)).astype(np.int32),
                        lasts=np.array([-1] + [int(c) for c in perm[:T - 1]], np.int32), actions=perm[:T].astype(np.int32)))
    return eps


def packed_buffer(S, episodes, max_eps, spare_plies=2):
    """The int32 hand-off buffer of include/af_engine.h af_engine_pack_episodes for these episodes:
        [0..3]                     episodes n, plies, K (key words per ply), C
        [4 + 4 i ..]               meta of episode i: game, sequence number, T, first ply index
        [4 + 4 max_eps + i]        final value of episode i (float bits)
        [4 + 5 max_eps + R p ..]   ply p, R = 2 K + 2 C + 2 ints: key (K u64, low half first) | policy float[C] | visits int[C] |
                                   last cell | action cell
    with `spare_plies` zeroed records behind the last one (an engine's buffer is sized for max_plies, not for what it holds)."""
    C, K = S * S, key_words(S)
    R = 2 * K + 2 * C + 2
    n, plies = len(episodes), sum(e["T"] for e in episodes)
    assert n <= max_eps
    buf = np.zeros(4 + 5 * max_eps + (plies + spare_plies) * R, np.uint32)
    buf[:4] = (n, plies, K, C)
    p0 = 0
    for i, e in enumerate(episodes):
        buf[4 + 4 * i:8 + 4 * i] = np.array([e["game"], e["seq"], e["T"], p0], np.int32).view(np.uint32)
        buf[4 + 4 * max_eps + i] = e["final_bits"]
        for t in range(e["T"]):
            rec = buf[4 + 5 * max_eps + (p0 + t) * R:][:R]
            rec[0:2 * K:2] = (e["keys"][t] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            rec[1:2 * K:2] = (e["keys"][t] >> np.uint64(32)).astype(np.uint32)
            rec[2 * K:2 * K + C] = e["policy_bits"][t]
            rec[2 * K + C:2 * K + 2 * C] = e["visits"][t].view(np.uint32)
            rec[2 * K + 2 * C] = np.int32(e["lasts"][t]).view(np.uint32)
            rec[2 * K + 2 * C + 1] = np.int32(e["actions"][t]).view(np.uint32)
        p0 += e["T"]
    return buf.view(np.int32)


def weight_table(max_T, gamma=GAMMA):
    """af_replay_set_weights' table: row T holds utils.construct_weights(T, gamma), float32[max_T + 1][max_T]"""
    from alphafive_amd import utils
    tab = np.zeros((max_T + 1, max_T), np.float32)
    for t in range(1, max_T + 1):
        tab[t, :t] = utils.construct_weights(t, gamma=gamma)
    return tab


def packed_expected(buf, max_eps, S, gamma=GAMMA):
    """What the ring must hold after each episode of `buf`: engine.unpack_episodes + engine.assemble_episode, the records'
    state strings decoded by utils.state_to_board -> per episode (boards int8[T,C], policies float32[T,C], last int32[T],
    values float32[T], weights float32[T])."""
    from alphafive_amd import engine, utils
    out = []
    for raw in engine.unpack_episodes(buf, max_eps):
        rec, _ = engine.assemble_episode(raw, S, gamma)
        out.append((np.stack([utils.state_to_board(r[0], S).reshape(-1) for r in rec]).astype(np.int8),
                    np.stack([r[1].reshape(-1) for r in rec]).astype(np.float32),
                    np.array([-1 if r[2] is None else r[2][0] * S + r[2][1] for r in rec], np.int32),
                    np.array([r[3] for r in rec], np.float32), np.array([r[4] for r in rec], np.float32)))
    return out


def packed_model(buf, max_eps, ep, T, S, wtab, fault=None):
    """af_replay_append_packed_kernel's decode of episode `ep` as the caller describes it (length T) -> the five arrays, or None
    where the kernel refuses (an episode the header does not hold, a length or a cell count other than the buffer's).
    `fault`: one of PACKED_FAULTS."""
    buf = np.ascontiguousarray(buf, np.int32)
    u = buf.view(np.uint32)
    n_eps, K, Cc = int(buf[0]), int(buf[2]), int(buf[3])
    C, max_T = S * S, wtab.shape[1]
    mT, p0 = int(buf[4 + 4 * ep + 2]), int(buf[4 + 4 * ep + 3])
    if ep >= n_eps or mT != T or Cc != C:
        return None
    R, KW = 2 * K + 2 * Cc + 2, K // 2
    boards, pol = np.zeros((T, C), np.int8), np.zeros((T, C), np.uint32)
    last, val, wts = np.zeros(T, np.int32), np.zeros(T, np.float32), np.zeros(T, np.float32)
    fv = u[4 + 4 * max_eps + ep:][:1].view(np.float32)[0]
    c = np.arange(C)
    w, b = c >> 6, c & 63
    if fault == "word_xor_1":
        w = w ^ 1
    half = 1 - (b >> 5) if fault == "halves_swapped" else b >> 5
    for t in range(T):
        o = 4 + 5 * max_eps + (p0 + t) * R
        key = u[o:o + R]
        mine = (key[2 * w + half] >> (b & 31).astype(np.uint32)) & 1
        theirs = (key[2 * (KW + w) + half] >> (b & 31).astype(np.uint32)) & 1
        if fault == "colours_swapped":
            mine, theirs = theirs, mine
        boards[t] = np.where(mine == 1, 1, np.where(theirs == 1, -1, 0))
        pol[t] = key[2 * K:2 * K + C]
        v = -fv if T & 1 else fv
        if (t + (1 if fault == "value_sign" else 0)) & 1:
            v = -v
        last[t] = buf[o + (R if fault == "last_of_next_ply" else 0) + 2 * K + 2 * C]
        val[t] = v
        wts[t] = wtab[T - 1 if fault == "weight_row" else T, t]
    return boards, pol.view(np.float32), last, val, wts
