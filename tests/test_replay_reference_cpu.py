"""tests/replay_cases.py without a GPU: the statements the device replay ring is held to (tests/test_gpu_replay_exact.py), the
conditions its generators promise, and that the comparisons reject the faults a kernel of pure data movement can have.

AUGMENTATION.  replay_cases.augment_reference equals tests/golden/replay_symmetries.npz (recorded from the unmodified reference,
tests/golden/make_replay_symmetries.py) at every S = 3..16, all 8 symmetries and last = none; and it equals
alphafive_amd.utils.RandomStack.get_data under dictated draws for every (S, last cell or none, k, flip): 12,040 cases.

GATHER.  At every S: the C + 1 boards have 8 pairwise distinct images each and differ from one another, policy values name their
(position, cell), values and weights are distinct, every (position, k, flip) triple occurs once, the ring's head is not 0 and the
cases cross its end; replay_cases.sample_model — the kernel's index arithmetic restated — equals augment_reference on all triples,
and with each planted fault (k taken as 4 - k, the flip before the turns, the last move left unturned, the last move turned the
inverse way, a horizontal flip in place of the vertical one, the slot taken without the head) the comparison reports a difference.

PACKED APPEND.  At S = 3, 8, 11, 12, 15, 16: the episode lengths are 1, 2, an odd and an even one, and C; the final values are
+1, -1, 0.0 and one arbitrary finite pattern; draws give -0.0 on alternate plies; every (cell, colour) pair occurs; each key word
that holds cells is non-zero at some ply and differs from every other one at some ply; the policies hold -0.0, subnormals and no
NaN or infinity.  replay_cases.packed_model — the kernel's decode restated — equals engine.unpack_episodes +
engine.assemble_episode, and with each planted fault (mine and theirs swapped, word w read as w ^ 1, the halves of a word swapped,
the value sign off by one ply, the weight row of T - 1, the last cell of the next ply) the comparison reports a difference.  The
model refuses what the kernel refuses.
"""
import os

import numpy as np
import pytest

import replay_cases as rc
from alphafive_amd import utils
from conftest import GOLDEN


def _fixture():
    return np.load(os.path.join(GOLDEN, "replay_symmetries.npz"))


@pytest.mark.parametrize("S", rc.SIZES)
def test_augment_reference_equals_the_reference_recording(S):
    z = _fixture()
    board, policy, last = rc.fixture_position(S)
    assert np.array_equal(board, z["board_%d" % S]) and rc.images_distinct(board) and last == 1
    assert z["boards_%d" % S].shape == (8, 3, S, S) and z["policies_%d" % S].shape == (8, S * S)
    for i, (k, f) in enumerate(rc.SYMMETRIES):
        got = rc.augment_reference(board, policy, last, k, f)
        assert not rc.differing(got, (z["boards_%d" % S][i], z["policies_%d" % S][i]), ("boards", "policies")), (k, f)
    k, f = (int(v) for v in z["none_symmetry"])
    for la in (-1, None):
        got = rc.augment_reference(board, policy, la, k, f)
        assert not rc.differing(got, (z["none_boards_%d" % S], z["none_policies_%d" % S]), ("boards", "policies"))
    assert not z["none_boards_%d" % S][2].any() and z["boards_%d" % S][:, 2].sum() == 8


@pytest.mark.parametrize("S", rc.SIZES)
def test_augment_reference_equals_the_host_class_on_every_cell_and_symmetry(S):
    boards, policies, last, values, weights, _ = rc.sample_cases(S)
    idx, turns, flip = rc.sample_triples(S)
    st = utils.RandomStack(S, length=10)
    st.data = rc.host_records(utils.board_to_state, boards, policies, last, values, weights)
    got = rc.scripted_get_data(st, idx, turns, flip)
    assert len(idx) == 8 * (S * S + 1)
    assert not rc.differing(got, rc.sample_expected(S), rc.SAMPLE_OUTPUTS)


def test_the_case_count():
    assert sum(8 * (S * S + 1) for S in rc.SIZES) == 12040 and max(8 * (S * S + 1) for S in rc.SIZES) == 2056


@pytest.mark.parametrize("S", rc.SIZES)
def test_gather_cases_keep_their_conditions(S):
    C = S * S
    boards, policies, last, values, weights, redraws = rc.sample_cases(S)
    assert boards.shape == (C + 1, C) and boards.dtype == np.int8 and set(np.unique(boards).tolist()) == {-1, 0, 1}
    assert all(rc.images_distinct(b.reshape(S, S)) for b in boards)
    assert len(set(b.tobytes() for b in boards)) == C + 1
    assert last.tolist() == list(range(C)) + [-1]
    assert policies.dtype == np.float32 and policies.max() == (C + 1) * C - 1 <= 65791 < 2 ** 24
    assert np.array_equal(policies.astype(np.int64), np.arange((C + 1) * C).reshape(C + 1, C))       # a value names (position, cell)
    assert len(set(values.tolist())) == C + 1 == len(set(weights.tolist()))
    assert np.array_equal(values.astype(np.float64) * 512, np.round(values.astype(np.float64) * 512))
    assert redraws == (3 if S == 3 else 0)             # distinct images are the rule: seeds 1000 + S redraw at S = 3 only
    idx, turns, flip = rc.sample_triples(S)
    assert sorted(zip(idx.tolist(), turns.tolist(), flip.tolist())) == [(p, k, f) for p in range(C + 1) for k in range(4) for f in (0, 1)]
    assert idx.tolist() != sorted(idx.tolist()) and len(idx) <= 2056
    ring, ops = rc.sample_ring(S)
    assert ring.head > 0 and ring.head + ring.count > ring.cap and ring.written.all()       # the cases cross the end of the ring
    assert not rc.differing(ring.logical(), rc.sample_cases(S)[:5], rc.FIELDS)
    assert [kind for kind, _ in ops] == ["append", "drop", "append", "drop", "append"]
    # what sits in the slots a head-less index would take is something else
    assert not np.array_equal(ring.boards[:C + 1], boards)


@pytest.mark.parametrize("S", rc.SIZES)
def test_gather_model_equals_the_statement_and_every_planted_fault_shows(S):
    ring, _ = rc.sample_ring(S)
    idx, turns, flip = rc.sample_triples(S)
    want = rc.sample_expected(S)
    assert not rc.differing(rc.sample_model(ring, idx, turns, flip), want, rc.SAMPLE_OUTPUTS)
    for fault in rc.SAMPLE_FAULTS:
        diff = rc.differing(rc.sample_model(ring, idx, turns, flip, fault=fault), want, rc.SAMPLE_OUTPUTS)
        assert diff, fault
        if fault.startswith("last_"):                  # the board and the policy are right there: only the third plane says so
            assert [d.split(":")[0] for d in diff] == ["boards"], (fault, diff)


def test_a_comparison_sees_one_bit_one_shape_and_one_type():
    a = np.zeros((4, 3), np.float32)
    b = a.copy()
    b[2, 1] = -0.0
    assert not rc.differing((a,), (a.copy(),), ("x",))
    assert rc.differing((a,), (b,), ("x",)) and "flat index 7" in rc.differing((a,), (b,), ("x",))[0]
    assert rc.differing((a,), (a.reshape(3, 4),), ("x",)) and rc.differing((a,), (a.astype(np.float64),), ("x",))


# ---------------------------------------------------------------------------------------------------------------------------
# packed hand-off buffers
# ---------------------------------------------------------------------------------------------------------------------------
MAX_EPS = 8


def _finite(bits):
    return ((bits >> np.uint32(23)) & np.uint32(0xFF)) != 0xFF


@pytest.mark.parametrize("S", rc.PACKED_SIZES)
def test_packed_episodes_keep_their_conditions(S):
    C, K = S * S, rc.key_words(S)
    KW, used = K // 2, (C + 63) // 64
    from alphafive_amd import engine
    assert K == engine.key_words(S) and (KW == 4) == (S >= 12)
    eps = rc.packed_episodes(S)
    T = [e["T"] for e in eps]
    assert T[0] == 1 and T[1] == 2 and T[4] == C and T[2] % 2 == 1 and T[3] % 2 == 0 and 2 < T[2] < C and 2 < T[3] < C
    assert len(eps) < MAX_EPS
    finals = np.array([e["final_bits"] for e in eps], np.uint32).view(np.float32)
    assert {1.0, -1.0, 0.0} <= set(finals.tolist()) and _finite(finals.view(np.uint32)).all()
    assert any(abs(v) not in (0.0, 1.0) for v in finals.tolist())
    # every (cell, colour) pair, every word that holds cells non-zero somewhere, every two words different somewhere
    seen = np.zeros((2, C), bool)
    words = np.concatenate([e["keys"] for e in eps])                  # [plies][K]
    for e in eps:
        for t in range(e["T"]):
            for col in (0, 1):
                for w in range(KW):
                    word = int(e["keys"][t, col * KW + w])
                    assert word >> max(0, min(64, C - 64 * w)) == 0          # no bit beyond the board
                    for b in range(64):
                        if word >> b & 1:
                            seen[col, 64 * w + b] = True
            assert not (e["keys"][t, :KW] & e["keys"][t, KW:]).any()       # no cell of both colours
            mine = sum(bin(int(x)).count("1") for x in e["keys"][t, :KW])
            theirs = sum(bin(int(x)).count("1") for x in e["keys"][t, KW:])
            assert mine + theirs == t and theirs - mine == t % 2           # the mover's opponent placed the last stone
    assert seen.all()
    live = [col * KW + w for col in (0, 1) for w in range(used)]
    assert all(words[:, w].any() for w in live)
    assert all((words[:, a] != words[:, b]).any() for a in live for b in live if a < b)
    assert not words[:, [col * KW + w for col in (0, 1) for w in range(used, KW)]].any()
    e = eps[4]
    assert sorted(e["actions"].tolist()) == list(range(C)) and e["lasts"][0] == -1 and np.array_equal(e["lasts"][1:], e["actions"][:-1])
    pol = np.concatenate([e["policy_bits"] for e in eps])
    assert _finite(pol).all()
    for special in rc.SPECIAL_POLICY_BITS:
        assert (pol == special).sum() >= 2                            # -0.0, +0.0, subnormals, the smallest normal, the largest finite values
    assert len(np.unique(pol)) > pol.size // 2

    buf = rc.packed_buffer(S, eps, MAX_EPS)
    raws = engine.unpack_episodes(buf, MAX_EPS)                          # the layout is the one the project reads
    assert len(raws) == len(eps) and buf.dtype == np.int32 and engine.packed_used_ints(buf[:4], MAX_EPS) < len(buf)
    for raw, e in zip(raws, eps):
        assert (raw["game"], raw["seq"], raw["T"]) == (e["game"], e["seq"], e["T"])
        assert np.float32(raw["final_value"]).view(np.uint32) == e["final_bits"]
        assert np.array_equal(raw["keys"], e["keys"]) and np.array_equal(raw["policies"].view(np.uint32), e["policy_bits"])
        assert np.array_equal(raw["visits"], e["visits"]) and np.array_equal(raw["lasts"], e["lasts"]) and np.array_equal(raw["actions"], e["actions"])
    assert [int(buf[4 + 4 * i + 3]) for i in range(len(eps))] == np.cumsum([0] + T[:-1]).tolist()     # first ply index > 0 but for one


@pytest.mark.parametrize("S", rc.PACKED_SIZES)
def test_packed_model_equals_the_host_records_and_every_planted_fault_shows(S):
    C = S * S
    eps = rc.packed_episodes(S)
    buf = rc.packed_buffer(S, eps, MAX_EPS)
    want = rc.packed_expected(buf, MAX_EPS, S)
    wtab = rc.weight_table(C)
    assert wtab.shape == (C + 1, C) and np.array_equal(wtab[C], utils.construct_weights(C, gamma=rc.GAMMA))
    for i, (e, w) in enumerate(zip(eps, want)):
        assert not rc.differing(rc.packed_model(buf, MAX_EPS, i, e["T"], S, wtab), w, rc.FIELDS), i
        assert set(np.unique(w[0]).tolist()) <= {-1, 0, 1} and (w[0] != 0).sum(axis=1).tolist() == list(range(e["T"]))
    # a draw alternates -0.0 and 0.0, as the host arithmetic gives them; the arbitrary value passes with its bits, signs alternating
    draw_bits = rc.bits(want[2][3]).tolist()
    assert draw_bits[:2] == [0x80000000, 0] and set(draw_bits) == {0, 0x80000000}            # T odd: -0.0 first
    assert set((rc.bits(want[3][3]) & 0x7FFFFFFF).tolist()) == {rc.ARBITRARY_FINAL}
    assert rc.bits(want[3][3]).tolist()[:2] == [rc.ARBITRARY_FINAL, rc.ARBITRARY_FINAL | 0x80000000]
    assert want[0][3].tolist() == [-1.0] and want[1][3].tolist() == [-1.0, 1.0]
    joined = tuple(np.concatenate([w[f] for w in want]) for f in range(5))
    for fault in rc.PACKED_FAULTS:
        got = [rc.packed_model(buf, MAX_EPS, i, e["T"], S, wtab, fault=fault) for i, e in enumerate(eps)]
        diff = rc.differing(tuple(np.concatenate([g[f] for g in got]) for f in range(5)), joined, rc.FIELDS)
        assert diff, fault
        field = {"value_sign": "values", "weight_row": "weights", "last_of_next_ply": "last"}.get(fault, "boards")
        assert [d.split(":")[0] for d in diff] == [field], (fault, diff)
    # what the kernel refuses: a length other than the buffer's, an episode the header does not hold, another board size
    assert rc.packed_model(buf, MAX_EPS, 2, eps[2]["T"] + 1, S, wtab) is None
    assert rc.packed_model(buf, MAX_EPS, len(eps), 1, S, wtab) is None
    other = buf.copy()
    other[3] = C + 1
    assert rc.packed_model(other, MAX_EPS, 0, 1, S, wtab) is None
