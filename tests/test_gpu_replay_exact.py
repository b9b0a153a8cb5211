"""The device replay ring (csrc/af_replay.hip: af_replay_sample_kernel, af_replay_append_packed_kernel, and af_replay_export_kernel
as the way to look at what they left) against independent numpy statements, bit for bit, through the C ABI of include/af_replay.h.
Every kernel here is pure data movement: a wrong index shows nowhere downstream, the net just learns from turned, recoloured or
misaligned positions.  Generators, statements and comparisons: tests/replay_cases.py; tests/test_replay_reference_cpu.py checks them
without a GPU, including that each comparison rejects the faults named below.  Nothing rounds, so there is no tolerance anywhere.

GATHER (af_replay_sample), every S = 3..16.  The statement is replay_cases.augment_reference — np.rot90 by k, then np.flip(axis 0),
of the three input planes and the policy alike, the last move's one-hot plane turning with the board — which
tests/golden/replay_symmetries.npz pins to the unmodified reference's get_data.  The kernel has two separately written pieces of
index arithmetic that must agree with it: the inverse map of the board (source_cell) and the forward map of the last move.
    positions   C + 1 per size: position p < C has its last move at cell p, position C has none; each on its own board whose 8 images
                are pairwise distinct; policy[p][c] = p C + c, so a value names its position and cell; value, weight distinct
    triples     all 8 (C + 1) (position, k, flip) in ONE call, in a fixed shuffled order (2,056 samples at S = 16, 80 at S = 3):
                sample index, position and symmetry are unrelated.  No (S, cell, symmetry) triple is left out: 12,040 in all
    sizes       S = 16 is C = 256 = the workgroup size (the cell loop runs exactly once; the memo's value slot once broke at C == 256),
                S = 3 and 4 are below one wave, S = 3..7 below 64 cells, even and odd boards alike
    the ring    every slot is first written with junk and dropped, then junk moves the head, so that head > 0 and the case
                positions cross the physical end: slot = (head + index) mod capacity, and what a head-less index would read is junk
    placement   the four outputs sit inside larger poisoned tensors: every word inside is written, none before or behind
    faults the comparison rejects at every S (CPU module): k taken as 4 - k, the flip before the turns, the last move left
                unturned or turned the inverse way, a horizontal flip, the slot taken without the head

PACKED APPEND (af_replay_append_packed), S = 3 (smallest), 8 (64 cells: one full key word), 11 (standard), 12 (144 cells, the first
size whose keys carry four words per colour: `key[2 * (KW + w) + (b >> 5)]` with KW = 4), 15 (the closed-loop board), 16 (every bit
of all four words).  The buffers are built word by word from the layout in include/af_engine.h (replay_cases.packed_buffer); what
the ring must hold is engine.unpack_episodes + engine.assemble_episode on the same array, which tests/test_host_utils.py pins to the
reference's records; the ring is read back with af_replay_export (boards, last cells, the bits of policies, values and weights).
    episodes    T = 1, 2, an odd and an even length in between, T = C (the full board = max_T, the last row of the weight table);
                final values +1, -1, 0.0 (a draw: -0.0 on alternate plies, as the host arithmetic gives) and one arbitrary finite
                pattern whose bits must pass; max_eps (8) above the episode count (5)
    stones      ply t holds the first t cells of the episode's permutation, colours alternating with the side to move: every
                (cell, colour) pair occurs, every key word that holds cells is non-zero at some ply and differs from every other
    policies    arbitrary finite bit patterns, -0.0, subnormals and the largest finite values among them; no NaN
    order       the even-length episode alone first, from the middle of the buffer (first ply index 3 or 10), wrapping the ring after
                its second ply; then all five in order, the head placed so that the T = C episode crosses the end half-way
    faults the comparison rejects (CPU module): mine and theirs swapped, word w read as w ^ 1, the 32-bit halves of a word swapped,
                the value sign off by one ply, the weight row of T - 1, the last cell of the next ply
    refusals    T < 1, T above the weight table, episode >= max_eps or < 0, a ring without a weight table: the argument error; an
                append past the capacity: the full error; none of them changes size or content.  A T other than the header's, and
                an episode index the header does not hold, make check() report once, and the slots keep their former bytes

THE REFERENCE'S OWN RECORDING.  The 60 episodes of tests/golden/randomstack.npz (recorded from the unmodified reference) pushed into
DeviceRandomStack(7, 400) under seed(21): accepted, data_len, result, the position count, black and white wins, the first and last
state through to_host(), the three 48-sample get_data batches bit for bit, and the next word of both random streams — the device
class against the reference in one hop.
"""
import contextlib
import ctypes as C
import io
import os
import random

import numpy as np
import pytest

import replay_cases as rc

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FULL, ERR_RANGE = 0, -1, -3, -4
POISON = 0x7FC0DEAD
MAX_EPS = 8


class _Ring(object):
    """A bare af_replay handle driven through ctypes, arrays in replay_cases.FIELDS order."""

    def __init__(self, S, cap):
        from alphafive_amd import replay
        self.L, self.S, self.C, self.h = replay.lib(), S, S * S, C.c_void_p()
        assert self.L.af_replay_create(S, cap, 0, C.byref(self.h)) == OK

    def size(self):
        return self.L.af_replay_size(self.h)

    def append(self, boards, policies, last, values, weights):
        a = [np.ascontiguousarray(x, t) for x, t in zip((boards, policies, last, values, weights),
                                                        (np.int8, np.float32, np.int32, np.float32, np.float32))]
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        return self.L.af_replay_append(self.h, None, len(a[2]), a[0].ctypes.data_as(C.POINTER(C.c_int8)), a[1].ctypes.data_as(fp),
                                       a[2].ctypes.data_as(ip), a[3].ctypes.data_as(fp), a[4].ctypes.data_as(fp))

    def drop(self, n):
        return self.L.af_replay_drop_front(self.h, n)

    def apply(self, mirror, kind, arg):
        """one append or drop on the device ring and on its host mirror"""
        assert (self.append(*arg) if kind == "append" else self.drop(arg)) == OK
        mirror.append(*arg) if kind == "append" else mirror.drop(arg)

    def move_head(self, mirror, n, seed):
        """junk in, junk out: the head moves on by n slots"""
        if n:
            self.apply(mirror, "append", rc.junk_positions(self.S, n, seed))
            self.apply(mirror, "drop", n)

    def export(self, first=0, n=None):
        n = self.size() - first if n is None else n
        bo, pol = np.full((n, self.C), 9, np.int8), np.full((n, self.C), np.nan, np.float32)
        last, val, wts = np.full(n, -9, np.int32), np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
        assert self.L.af_replay_export(self.h, None, first, n, None, bo.ctypes.data, pol.ctypes.data, last.ctypes.data,
                                       val.ctypes.data, wts.ctypes.data) == OK
        return bo, pol, last, val, wts

    def set_weights(self, tab):
        tab = np.ascontiguousarray(tab, np.float32)
        return self.L.af_replay_set_weights(self.h, tab.ctypes.data_as(C.POINTER(C.c_float)), tab.shape[1])

    def append_packed(self, dev, max_eps, ep, T):
        return self.L.af_replay_append_packed(self.h, None, dev.data_ptr(), max_eps, ep, T)

    def check(self):
        return self.L.af_replay_check(self.h, None)

    def close(self):
        self.L.af_replay_destroy(self.h)


# ---------------------------------------------------------------------------------------------------------------------------
# the gather kernel on every symmetry, every cell, every size
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", rc.SIZES)
def test_gather_equals_the_augmentation_on_every_cell_and_symmetry(S):
    import torch
    Cc = S * S
    mirror, ops = rc.sample_ring(S)
    ring, twin = _Ring(S, mirror.cap), rc.RingMirror(S, mirror.cap)
    for kind, arg in ops:
        ring.apply(twin, kind, arg)
    assert ring.size() == Cc + 1 and twin.head == mirror.head > 0 and twin.head + Cc + 1 > twin.cap
    assert not rc.differing(ring.export(), rc.sample_cases(S)[:5], rc.FIELDS)            # the ring holds the cases, across its end
    idx, turns, flip = rc.sample_triples(S)
    N, pad = len(idx), 512
    assert N == 8 * (Cc + 1)
    sizes = [N * 3 * Cc, N, N, N * Cc]
    bufs = [torch.full((sz + 2 * pad,), POISON, dtype=torch.int32, device="cuda") for sz in sizes]
    torch.cuda.synchronize()
    ip = C.POINTER(C.c_int32)
    assert ring.L.af_replay_sample(ring.h, None, N, idx.ctypes.data_as(ip), turns.ctypes.data_as(ip), flip.ctypes.data_as(ip),
                                   *[b.data_ptr() + 4 * pad for b in bufs]) == OK
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h, sz in zip(host, sizes):
        assert (h[:pad] == POISON).all() and (h[pad + sz:] == POISON).all()                # nothing before, nothing behind
        assert not (h[pad:pad + sz] == POISON).any()                                       # every word inside was written
    shapes = [(N, 3, S, S), (N,), (N,), (N, Cc)]
    got = [h[pad:pad + sz].view(np.float32).reshape(shape) for h, sz, shape in zip(host, sizes, shapes)]
    assert not rc.differing(got, rc.sample_expected(S), rc.SAMPLE_OUTPUTS)
    assert not rc.differing(ring.export(), rc.sample_cases(S)[:5], rc.FIELDS)            # sampling left the ring as it was
    ring.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the packed append on crafted hand-off buffers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", rc.PACKED_SIZES)
def test_packed_append_equals_the_host_records(S):
    import torch
    Cc = S * S
    eps = rc.packed_episodes(S)
    n = len(eps)
    buf = rc.packed_buffer(S, eps, MAX_EPS).copy()
    want = rc.packed_expected(buf, MAX_EPS, S)
    buf[4 + 4 * n:8 + 4 * n] = buf[4:8]                # meta of an episode the header does not count: episode 0's, so that only
    buf[4 + 4 * MAX_EPS + n] = buf[4 + 4 * MAX_EPS]    # the count refuses it (further down)
    T = [e["T"] for e in eps]
    total = sum(T)
    cap = total + 3
    ring, mirror = _Ring(S, cap), rc.RingMirror(S, cap)
    dev = torch.from_numpy(buf).cuda()
    assert ring.append_packed(dev, MAX_EPS, 0, T[0]) == ERR_ARG and ring.size() == 0      # no weight table yet
    assert ring.set_weights(rc.weight_table(Cc)) == OK
    ring.move_head(mirror, cap, 7000 + S)              # every slot holds known bytes from here on

    # the even-length episode alone, from the middle of the buffer, wrapping after its second ply
    ring.move_head(mirror, cap - 2, 7100 + S)
    assert int(buf[4 + 4 * 3 + 3]) == T[0] + T[1] + T[2] > 0 and mirror.head == cap - 2
    assert ring.append_packed(dev, MAX_EPS, 3, T[3]) == OK
    mirror.append(*want[3])
    assert ring.check() == OK and ring.size() == T[3]
    assert not rc.differing(ring.export(), want[3], rc.FIELDS)
    ring.apply(mirror, "drop", T[3])

    # all five in order, the T = C episode crossing the end of the ring half-way
    head = cap - sum(T[:4]) - Cc // 2
    ring.move_head(mirror, (head - mirror.head) % cap, 7200 + S)
    assert mirror.head == head and head + sum(T[:4]) < cap < head + total
    for i in range(n):
        assert ring.append_packed(dev, MAX_EPS, i, T[i]) == OK
        mirror.append(*want[i])
    assert ring.check() == OK and ring.size() == total
    stored = tuple(np.concatenate([w[f] for w in want]) for f in range(5))
    assert not rc.differing(ring.export(), stored, rc.FIELDS)
    for i in (0, 2, 4):                                # ... and read out episode by episode, from a first position > 0
        assert not rc.differing(ring.export(sum(T[:i]), T[i]), want[i], rc.FIELDS), i

    # refusals: nothing moves, nothing is written
    assert ring.append_packed(dev, MAX_EPS, 4, T[4]) == ERR_FULL                           # 3 slots are free
    for ep, t in ((0, 0), (0, -1), (4, Cc + 1), (MAX_EPS, 1), (-1, 1)):
        assert ring.append_packed(dev, MAX_EPS, ep, t) == ERR_ARG, (ep, t)
    assert ring.L.af_replay_append_packed(ring.h, None, None, MAX_EPS, 0, 1) == ERR_ARG
    assert ring.size() == total and ring.check() == OK
    assert not rc.differing(ring.export(), stored, rc.FIELDS)

    # a length other than the header's, an episode the header does not hold: the host cannot know, check() reports, and the
    # slots keep their former bytes
    ring.apply(mirror, "drop", sum(T[:3]))
    assert ring.append_packed(dev, MAX_EPS, 2, T[2] + 1) == OK
    mirror.skip(T[2] + 1)
    assert ring.check() == ERR_RANGE and ring.check() == OK                                # reported once
    assert ring.append_packed(dev, MAX_EPS, n, 1) == OK
    mirror.skip(1)
    assert ring.check() == ERR_RANGE and ring.check() == OK
    assert ring.size() == mirror.count
    assert not rc.differing(ring.export(), mirror.logical(), rc.FIELDS)
    # ... and the ring goes on working
    assert ring.append_packed(dev, MAX_EPS, 1, T[1]) == OK
    mirror.append(*want[1])
    assert ring.check() == OK
    assert not rc.differing(ring.export(), mirror.logical(), rc.FIELDS)
    ring.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's own recording through the device class
# ---------------------------------------------------------------------------------------------------------------------------
def test_device_randomstack_matches_the_reference_recording(golden_dir):
    from alphafive_amd.replay import DeviceRandomStack
    z = dict(np.load(os.path.join(golden_dir, "randomstack.npz")))
    S, length = int(z["S"]), int(z["length"])
    assert (S, length, int(z["n_episodes"])) == (7, 400, 60)
    np.random.seed(21)
    random.seed(21)
    st = DeviceRandomStack(S, length, device=0)
    accepted = []
    with contextlib.redirect_stdout(io.StringIO()):
        for e in range(int(z["n_episodes"])):
            recs = []
            for t in range(len(z[f"ep{e}_states"])):
                la = int(z[f"ep{e}_lasts"][t])
                recs.append((str(z[f"ep{e}_states"][t]), z[f"ep{e}_policies"][t], None if la < 0 else (la // S, la % S),
                             float(z[f"ep{e}_values"][t]), np.float32(z[f"ep{e}_weights"][t])))
            accepted.append(st.push(recs, int(z[f"ep{e}_result"])))
    assert accepted == list(z["accepted"])
    assert st.data_len == list(z["data_len"]) and st.result == list(z["result"])
    assert st._size() == int(z["n_data"]) and st.is_full() == (st._size() >= st.length)
    assert (st.black_win, st.white_win) == (int(z["black_win"]), int(z["white_win"]))
    host = st.to_host()
    assert len(host.data) == int(z["n_data"])
    assert host.data[0][0] == str(z["first_state"]) and host.data[-1][0] == str(z["last_state"])
    for b in range(3):
        got = [t.cpu().numpy() for t in st.get_data(batch_size=48)]
        want = [z[f"batch{b}_{k}"] for k in rc.SAMPLE_OUTPUTS]
        assert got[0].shape == (48, 3, S, S) and got[3].shape == (48, S * S)
        assert not rc.differing(got, want, rc.SAMPLE_OUTPUTS), b
    assert int(np.random.randint(0, 2 ** 32, dtype=np.uint64)) == int(z["np_next"])
    assert random.getrandbits(32) == int(z["py_next"])
    st.close()
