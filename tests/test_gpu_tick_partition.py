"""All eight instantiations of af_tick_kernel<KW, W64, MEMO> against the C oracle on searches that descend (tests/tick_cases.py), under
every way of cutting a game's work into launches: the per-launch select budget (yield at the next simulation boundary), the hard cap
(yield inside a descent, resume from the stored position, depth, last move and path), the memo's own budget and the collector's
yield.  include/af_engine.h says of the budget "Results do not depend on it": here that is a test.  Also the contract of the leaf
batch: a tick writes planes[g] only for the games it parks and reads policy[g] / value[g] only of the games it left parked.

Everything compared is an integer or a bit pattern; nothing takes a tolerance.  Budgets from the environment are set before the
engine is created (af_engine_create and af_engine_memo_enable read them once)."""
import time

import numpy as np
import pytest

import tick_cases as tc
from test_gpu_parity import _compare_tree

pytestmark = pytest.mark.gpu

ENV = ("AF_TICK_BUDGET", "AF_TICK_BUDGET_HARD", "AF_MEMO_BUDGET")
# id -> (environment, set_tick_budget argument or None, soft budget, hard cap)
BUDGETS = {
    "1_1": (dict(AF_TICK_BUDGET="1", AF_TICK_BUDGET_HARD="1"), None, 1, 1),
    "1_12": ({}, 1, 1, 12),
    "2_3": (dict(AF_TICK_BUDGET="2", AF_TICK_BUDGET_HARD="3"), None, 2, 3),
    "default": ({}, None, 8, 12),
    "never": (dict(AF_TICK_BUDGET="100000"), None, 100000, 100000),
}
SMALL = ("1_1", "1_12", "2_3")


def _set_budget_env(monkeypatch, budget, memo_budget=None):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in BUDGETS[budget][0].items():
        monkeypatch.setenv(k, v)
    if memo_budget is not None:
        monkeypatch.setenv("AF_MEMO_BUDGET", str(memo_budget))


def _assert_episode(raw, ref, S, gamma, what):
    from alphafive_amd.engine import assemble_episode
    orec = ref["records"]
    assert raw["seq"] == 0 and raw["T"] == len(orec), what
    assert (raw["actions"] == ref["actions"]).all(), what
    assert (raw["visits"] == ref["visits"]).all(), what
    assert raw["final_value"] == ref["final_value"], what
    rec, _ = assemble_episode(raw, S, gamma)
    for (s, p, la, v, w), (os_, op, ola, ov, ow) in zip(rec, orec):
        assert s == os_ and la == ola and v == ov and w == ow, what
        assert (p.view(np.uint32) == op.view(np.uint32)).all(), what


def _tick_bound(refs):
    """Ticks after which every game has handed over its first episode whatever the budget: a tick that does not finish a simulation
    does a select or runs the collector, so four times the oracle's selects + simulations of the longest game is generous."""
    return 4 * max(e["stats"]["selects"] + e["stats"]["sims"] for e in refs) + 1024


def _first_episodes(monkeypatch, name, value_f64, memo, budget, hyper=None, memo_budget=None, graph=False):
    """SelfPlayEngine on the case until every game has handed over its first episode -> what the run did; the episodes are compared
    with the oracle's here."""
    from alphafive_amd import engine as eng
    from alphafive_amd.engine import SelfPlayEngine
    case = tc.CASES[name]
    refs = tc.episodes(name, value_f64, hyper)
    _set_budget_env(monkeypatch, budget, memo_budget)
    cfg = tc.cfg_of(case, hyper)
    kw = dict(eval_memo=dict(log2_buckets=case.log2_buckets, max_stones=case.max_stones), weights_version=0) if memo else {}
    t0 = time.time()
    sp = SelfPlayEngine(cfg, case.G, tc.pv_torch(case), device=0, seed=case.seed, first_game_id=case.first, value_f64=value_f64, **kw)
    try:
        assert sp.engine.KW2 == case.kw2 == eng.key_words(case.S)
        if BUDGETS[budget][1] is not None:
            sp.engine.set_tick_budget(BUDGETS[budget][1])
        sp.engine.tick_histogram(reset=True)
        eps, bound = {}, _tick_bound(refs)
        while len(eps) < case.G and sp.ticks < bound:
            if graph:
                for _ in range(16):
                    sp.run_ticks_graph(16)
            else:
                sp.run_ticks(256)
            sp.check()
            for raw in sp.pop_raw(cap=64):
                eps.setdefault(raw["game"], raw)
        assert len(eps) == case.G, "games without a first episode after %d ticks: %s" % (sp.ticks, sorted(set(range(case.G)) - set(eps)))
        sp.check()
        ct, hist = sp.counters(), sp.engine.tick_histogram()
        ms = sp.engine.memo_stats() if memo else None
        ticks = sp.ticks
        if graph:
            assert sp._graph is not None
    finally:
        sp.close()
    took = time.time() - t0
    sel = hist["selects"]
    print("tick-partition", name, "f64" if value_f64 else "f32", "memo" if memo else "plain", budget, "hyper2" if hyper else "",
          "memo_budget=%s" % memo_budget, "graph" if graph else "eager", "ticks", ticks, "%.2fs" % took,
          {k: ct[k] for k in ("sims", "selects", "expands", "terminals", "yields", "collector_runs", "plies", "episodes")},
          "selects/launch", {int(i): int(sel[i]) for i in np.flatnonzero(sel)}, "memo", ms)
    for g in range(case.G):
        _assert_episode(eps[g], refs[g], case.S, cfg.gamma, (name, value_f64, memo, budget, g))
    # the path this run is there for was taken
    _, _, soft, hard = BUDGETS[budget]
    # no launch did more selects than the hard cap (with the budget that never yields the cap lies beyond the histogram's 64 bins and
    # the slice is empty: nothing is claimed there)
    assert sel[hard + 1:].sum() == 0
    assert ct["sims"] == ct["expands"] + ct["terminals"] and ct["terminals"] > 0 and ct["stalls"] == 0
    if budget == "1_1":
        assert sel[2:].sum() == 0 and ct["selects"] > ct["sims"]   # some simulation needed two selects: resumed from memory
    if budget == "default":
        assert sel[2:].sum() > 0
    if budget in SMALL:
        assert ct["yields"] > 0
    if memo:
        assert ms["hits"] > 0 and ms["replaced"] > 0, ms
    if case.kw2 == 8:
        assert ct["collector_runs"] > 0                            # the default store (4 sims + 64 nodes) came under pressure
    return dict(counters=ct, hist=hist, memo=ms, ticks=ticks)


# ---- a. episodes under every budget, every instantiation ----
@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("memo", [False, True], ids=["plain", "memo"])
@pytest.mark.parametrize("value_f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_first_episodes_equal_the_oracle_under_every_budget(monkeypatch, name, value_f64, memo, budget):
    _first_episodes(monkeypatch, name, value_f64, memo, budget)


@pytest.mark.parametrize("name,value_f64", [("kw2", False), ("kw4", True)])
def test_first_episodes_equal_the_oracle_with_a_memo_budget_of_one(monkeypatch, name, value_f64):
    """AF_MEMO_BUDGET=1 under the default select budget: a game that has consumed a memo hit yields after its first select."""
    out = _first_episodes(monkeypatch, name, value_f64, True, "default", memo_budget=1)
    assert out["counters"]["yields"] > 0


@pytest.mark.parametrize("memo", [False, True], ids=["plain", "memo"])
@pytest.mark.parametrize("value_f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_first_episodes_equal_the_oracle_with_other_hyper_parameters(monkeypatch, name, value_f64, memo):
    """c_puct = 1.5, dirichlet_alpha = 0.15 at 2 / 3: launches of one to three selects, yields at boundaries and inside descents."""
    _first_episodes(monkeypatch, name, value_f64, memo, "2_3", hyper=tc.HYPER2)


@pytest.mark.parametrize("name,value_f64", [("kw2", False), ("kw4", True)])
def test_first_episodes_equal_the_oracle_inside_the_graph_loop_at_one_select_per_launch(monkeypatch, name, value_f64):
    _first_episodes(monkeypatch, name, value_f64, True, "1_1", graph=True)


# ---- b. trees under the extreme budgets ----
@pytest.mark.parametrize("budget", ["1_1", "default"])
@pytest.mark.parametrize("value_f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_trees_after_three_moves_equal_the_oracle(monkeypatch, name, value_f64, budget):
    """Engine in MODE_EXTERNAL driven by hand: every move against OraclePlayer.get_action (action, visits, policy bits, tau), then the
    whole tree (N, W bits — the fp64 rows with the fp64 store —, the fp32-typed flag, P bits, sum_n)."""
    import torch
    from alphafive_amd import engine as eng
    case = tc.CASES[name]
    S, C, G = case.S, case.S * case.S, tc.TRACE_GAMES
    traces = tc.trace(name, value_f64)
    _set_budget_env(monkeypatch, budget)
    t0 = time.time()
    e = eng.Engine(tc.cfg_of(case), G, mode=eng.MODE_EXTERNAL, training=True, seed=case.seed, first_game_id=case.first,
                   value_f64=value_f64)
    try:
        e.tick_histogram(reset=True)
        pv = tc.pv_torch(case)
        planes = torch.zeros((G, 3, S, S), device="cuda")
        pol, val = torch.zeros((G, C), device="cuda"), torch.zeros((G,), device="cuda")
        ticks = 0
        for mv in range(tc.TRACE_MOVES):
            games = [g for g in range(G) if mv < len(traces[g]["moves"])]          # a game that ended stops there
            if not games:
                break
            for g in games:
                m = traces[g]["moves"][mv]
                lc = -1 if m["last"] is None else m["last"][0] * S + m["last"][1]
                e.set_root(g, eng.state_to_key(m["state"], S), lc, random_a=False, reset_tree=(mv == 0))
            bound = ticks + 4 * (2 * case.cap + 64) * 8
            while True:
                e.tick(pol.data_ptr(), val.data_ptr(), planes.data_ptr())
                ticks += 1
                st = e.status()
                if all(st[g] == eng.STATUS_MOVE_DONE for g in games):
                    break
                assert ticks < bound, "move %d not decided" % mv
                pr, va = pv(planes)
                pol.copy_(pr.reshape(G, -1))
                val.copy_(va.reshape(G))
            for g in games:
                m = traces[g]["moves"][mv]
                cell, po, vi, tau = e.move_result(g)
                assert cell == m["cell"] and tau == m["tau"], (g, mv)
                np.testing.assert_array_equal(vi, m["visits"])
                assert po is not None
                np.testing.assert_array_equal(po.view(np.uint32), m["policy"].reshape(-1).view(np.uint32))
        ct, hist = e.counters(), e.tick_histogram()
        nodes = 0
        for g in range(G):
            seen, total = _compare_tree(e.tree_dump(g), traces[g]["tree"], S)
            nodes += seen
    finally:
        e.close()
    print("tick-partition trees", name, "f64" if value_f64 else "f32", budget, "ticks", ticks, "%.2fs" % (time.time() - t0),
          "nodes compared", nodes, {k: ct[k] for k in ("sims", "selects", "yields")})
    sel = hist["selects"]
    assert sel[BUDGETS[budget][3] + 1:].sum() == 0
    if budget == "1_1":
        assert ct["selects"] > ct["sims"] and ct["yields"] > 0
    else:
        assert sel[2:].sum() > 0


def test_player_host_loop_sees_yields_inside_a_descent(monkeypatch):
    """Player(pv_fn=...) on 6x6 at 1 / 1: the host loop's STATUS_YIELD branch gets yields that come from inside a descent."""
    from alphafive_amd.player import Player
    case = tc.CASES["kw2"]
    tr = tc.trace("kw2", False)[0]
    _set_budget_env(monkeypatch, "1_1")
    pl = Player(tc.cfg_of(case), training=True, pv_fn=tc.pv_np(case), seed=case.seed, game_id=case.first)
    try:
        pl.reset()                                     # as the trace: the first root is installed with reset_tree
        pl._engine.tick_histogram(reset=True)
        for m in tr["moves"]:
            pol, act = pl.get_action(m["state"], last_action=m["last"])
            assert act[0] * case.S + act[1] == m["cell"] and pl.tau == m["tau"]
            assert (pl.last_visits == m["visits"]).all()
            assert (pol.view(np.uint32) == m["policy"].view(np.uint32)).all()
        _compare_tree(pl._engine.tree_dump(0), tr["tree"], case.S)
        ct, hist = pl._engine.counters(), pl._engine.tick_histogram()
        assert hist["selects"][2:].sum() == 0 and ct["selects"] > ct["sims"] and ct["yields"] > 0
    finally:
        pl.close()


def test_device_arena_at_one_select_per_launch_equals_its_yardstick(monkeypatch):
    """The s6 arena shape of test_gpu_arena_device (eval mode, random_a): play_matches_device at 1 / 1 against play_matches at the
    default budget."""
    from alphafive_amd import arena
    import test_gpu_arena_device as ad
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    want = ad._yardstick("s6_kw2_both_sides_win")
    S, goal, G, sims, upper, max_plies, nets = ad.SHAPES["s6_kw2_both_sides_win"]
    _set_budget_env(monkeypatch, "1_1")
    pv = ad._pvs(nets)
    got = arena.play_matches_device(ad._cfg(S, goal, sims, upper), pv[0], pv[1], G, seed0=ad.SEEDS[0], seed1=ad.SEEDS[1],
                                    max_plies=max_plies, graph=False)
    for k in ad.KEYS:
        assert got[k] == want[k], k


# ---- c. the leaf-batch contract ----
SENTINEL = -7.0


@pytest.mark.parametrize("budget", ["default", "1_1"])
@pytest.mark.parametrize("memo", [False, True], ids=["plain", "memo"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_a_tick_writes_and_reads_only_the_rows_of_parked_games(monkeypatch, name, memo, budget):
    """The tick / forward / insert loop written out: planes are poisoned before every tick, the evaluations of every game that is
    not at NEED_EVAL are NaN when the insert and the next tick run.  The episodes are the oracle's all the same (so no NaN ever
    reached a tree, through the memo or otherwise), and what a tick leaves in `planes` is what the contract says."""
    import torch
    from alphafive_amd import engine as eng
    from alphafive_amd.engine import unpack_episodes
    case = tc.CASES[name]
    S, C = case.S, case.S * case.S
    # this loop reads the status after every tick, and a four-word game at one select per launch takes 1.6 times the ticks of its
    # default-budget twin (profiles/tick_partition.md): that case runs four of the eight games
    G = 4 if (name, budget) == ("kw4", "1_1") else case.G
    refs = tc.episodes(name, False)[:G]
    _set_budget_env(monkeypatch, budget)
    cfg = tc.cfg_of(case)
    t0 = time.time()
    e = eng.Engine(cfg, G, mode=eng.MODE_SELFPLAY, training=True, seed=case.seed, first_game_id=case.first)
    try:
        if memo:
            e.memo_enable(case.log2_buckets, case.max_stones)
        pv = tc.pv_torch(case)
        planes = torch.zeros((G, 3, S, S), device="cuda")
        pol, val = torch.zeros((G, C), device="cuda"), torch.zeros((G,), device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        cap, max_plies = 64, max(64 * 40, e.max_plies)
        box = torch.zeros(e.pack_ints(cap, max_plies), dtype=torch.int32, device="cuda")
        eps, ticks, bound = {}, 0, _tick_bound(refs)
        parked_rows = 0
        while len(eps) < G:
            assert ticks < bound, "games without a first episode: %s" % sorted(set(range(G)) - set(eps))
            planes.fill_(SENTINEL)                                             # 1
            e.tick(pol.data_ptr(), val.data_ptr(), planes.data_ptr(), stream)   # 2
            ticks += 1
            need = e.status(stream) == eng.STATUS_NEED_EVAL                    # 3
            # what the tick left in planes (read on the host: the status read has drained the stream anyway): the sentinel for every
            # game it did not park; for a parked game 0 / 1 only, no cell in both stone planes, the last move empty or one cell, and
            # that cell an opponent stone
            rows = planes.cpu().numpy().reshape(G, 3, C)
            assert (rows[~need] == SENTINEL).all(), "tick %d: planes of a game that is not at NEED_EVAL were written" % ticks
            pr = rows[need]
            parked_rows += len(pr)
            one = pr == 1
            assert (one | (pr == 0)).all(), "tick %d: a parked row holds something other than 0 and 1" % ticks
            assert not (one[:, 0] & one[:, 1]).any(), "tick %d: a cell is set in both stone planes" % ticks
            assert (one[:, 2].sum(axis=1) <= 1).all(), "tick %d: more than one last move" % ticks
            assert not (one[:, 2] & ~one[:, 1]).any(), "tick %d: the last move is not an opponent stone" % ticks
            p, v = pv(planes)                                                  # 4
            pol.copy_(p.reshape(G, C))
            val.copy_(v.reshape(G))
            idle = torch.from_numpy(~need).to("cuda")
            pol.masked_fill_(idle[:, None], float("nan"))                      # 5
            val.masked_fill_(idle, float("nan"))
            if memo:
                e.memo_insert(pol.data_ptr(), val.data_ptr(), stream)          # 6
            if ticks % 256 == 0:
                e.pack_episodes(box.data_ptr(), cap, max_plies, stream)
                for raw in unpack_episodes(box.cpu().numpy(), cap):
                    eps.setdefault(raw["game"], raw)
        ct = e.counters(stream)
        ms = e.memo_stats(stream) if memo else None
    finally:
        e.close()
    print("tick-partition leaf batch", name, "memo" if memo else "plain", budget, "ticks", ticks, "%.2fs" % (time.time() - t0),
          "parked rows checked", parked_rows, {k: ct[k] for k in ("sims", "selects", "yields")}, "memo", ms)
    for g in range(G):
        _assert_episode(eps[g], refs[g], S, cfg.gamma, (name, memo, budget, g))
    assert parked_rows > 0
    if memo:
        assert ms["hits"] > 0 and ms["inserts"] > 0
    if budget == "1_1":
        assert ct["selects"] > ct["sims"] and ct["yields"] > 0
