"""Batched checkpoint arena — the match loop of the reference's choose_best_player.py:38-60 for many
games at once (a caller of the hot path).

Reference protocol, per game i: both players are reset (:43-44), player (i % 2) moves first (:48), players
alternate, each calling get_action(state, last_action=action, random_a=True) on its OWN tree with
training=False (:32-33,52) — temperature play with tau *= tau_decay_rate_r per own move (player.py:108-109) —
until is_game_over; a non-draw is a win for the player who just moved (:62-63).

Here every game is one slot of two EXTERNAL-mode engines (one per player / weight set).  At ply k the mover
of game i is player (i + k) % 2, so each ply activates the even games in one engine and the odd games in the
other; a mover's engine runs its tick loop (tree kernel -> leaf batch -> its own net) until all of its active
games have decided their move.
"""
import ctypes

import numpy as np

from . import engine as _eng
from . import utils


def play_matches(cfg, pv0, pv1, n_games, device=0, seed0=0, seed1=1, node_cap=0, max_plies=None):
    """pv0 / pv1: device evaluators (planes float32[G,3,S,S] -> (prob[G,C], value[G]) torch tensors).
    Returns dict(wins=[w0, w1], draws, moves=[[cell,...] per game], lengths)."""
    import torch
    S, G = cfg.board_size, n_games
    C = S * S
    dev = torch.device("cuda", device)
    engines = [_eng.Engine(cfg, G, device=device, mode=_eng.MODE_EXTERNAL, training=False, seed=s, node_cap=node_cap)
               for s in (seed0, seed1)]
    pvs = [pv0, pv1]
    planes = torch.zeros((G, 3, S, S), dtype=torch.float32, device=dev)
    policy = [torch.zeros((G, C), dtype=torch.float32, device=dev) for _ in range(2)]
    value = [torch.zeros((G,), dtype=torch.float32, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    boards = [np.zeros((S, S), np.int8) for _ in range(G)]
    last = [None] * G
    over = [False] * G
    moves = [[] for _ in range(G)]
    wins, draws = [0, 0], 0
    ply = 0
    limit = max_plies or C
    while not all(over) and ply < limit:
        for p in (0, 1):
            active = [i for i in range(G) if not over[i] and (i + ply) % 2 == p]
            if not active:
                continue
            e = engines[p]
            keys = np.stack([_eng.state_to_key(utils.board_to_state(boards[i]), S) for i in active])
            lcs = [-1 if last[i] is None else last[i][0] * S + last[i][1] for i in active]
            e.set_roots(active, keys, lcs, random_a=True, reset_tree=(ply < 2), stream=stream)   # Player.reset() before each game
            while True:
                e.tick(policy[p].data_ptr(), value[p].data_ptr(), planes.data_ptr(), stream)
                st = e.status(stream)
                if all(st[i] == _eng.STATUS_MOVE_DONE for i in active):
                    break
                pr, va = pvs[p](planes)
                policy[p].copy_(pr.reshape(G, C))
                value[p].copy_(va.reshape(G))
            cells = e.move_results(active, stream=stream)[0]
            for i, cell in zip(active, cells):
                cell = int(cell)
                a = (cell // S, cell % S)
                moves[i].append(cell)
                boards[i] = utils.step(boards[i], a)
                last[i] = a
                done, v = utils.is_game_over(boards[i], cfg.goal)
                if done:
                    over[i] = True
                    if v == 0.0:
                        draws += 1
                    else:
                        wins[p] += 1                     # the player who just moved (choose_best_player.py:62-63)
        ply += 1
    for e in engines:
        e.close()
    return dict(wins=wins, draws=draws, moves=moves, lengths=[len(m) for m in moves])


# ---- the same match without the host in the loop ----
MATCH_WIN0, MATCH_WIN1, MATCH_DRAW, MATCH_UNFINISHED = 0, 1, 2, -1          # af_engine.h AF_MATCH_*
TICK_SLACK = 64       # run()'s bound: ticks per move beyond 2 * upper_simulation_per_step (move start, collector runs, the lagged poll)


class DeviceArena:
    """play_matches with both players' engines ticking all the time and the hand-over of a decided move — append it, play it, game
    over?, tally, set the opponent's root — done by one small kernel (af_engine.h af_match_step) instead of the host.

    One ROUND is: tick of engine 0, forward of net 0, step, tick of engine 1, forward of net 1, step, on torch's current stream.
    A tick returns at once for a game whose player has nothing to search, and the forward evaluates all G slots whether their game
    is waiting for it or not (it is slot-independent to the bit, and play_matches evaluates all G slots too), so nothing in a round
    depends on the state of the match: run() replays rounds_per_replay of them as one HIP graph and looks at three progress words,
    one replay late.  Every game is a function of the two seeds and the two nets only — the same moves as play_matches, to the cell.

    pv0 / pv1: device evaluators as for play_matches; one that takes bind_outputs writes straight into its player's tensors.
    weights_versions: per player, what SelfPlayEngine(weights_version=) takes, for evaluators that hide their net in a wrapper."""

    def __init__(self, cfg, pv0, pv1, num_games, device=0, seed0=0, seed1=1, node_cap=0, weights_versions=(None, None)):
        import torch
        if not torch.cuda.is_available():
            raise _eng.EngineError("DeviceArena needs a HIP device (torch.cuda.is_available() is False)")
        self.torch = torch
        self.cfg = cfg
        S, G = cfg.board_size, num_games
        self.S, self.C, self.G = S, S * S, G
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.engines, self._match = [], None
        for s in (seed0, seed1):
            self.engines.append(_eng.Engine(cfg, G, device=device, mode=_eng.MODE_EXTERNAL, training=False, seed=s, node_cap=node_cap))
        h = ctypes.c_void_p()
        _eng._check(_eng.lib().af_match_create(self.engines[0]._h, self.engines[1]._h, ctypes.byref(h)), "af_match_create")
        self._match = h
        self.pvs = [pv0, pv1]
        self.planes = [torch.zeros((G, 3, S, S), dtype=torch.float32, device=self.dev) for _ in range(2)]
        self.policy = [torch.zeros((G, self.C), dtype=torch.float32, device=self.dev) for _ in range(2)]
        self.value = [torch.zeros((G,), dtype=torch.float32, device=self.dev) for _ in range(2)]
        self._versions, self._version_missing = [], False
        for p, pv in enumerate(self.pvs):
            ver, missing = _eng.resolve_weights_version(pv, weights_versions[p])
            self._versions.append(ver)
            self._version_missing = self._version_missing or missing
            if hasattr(pv, "bind_outputs"):
                pv.bind_outputs(self.policy[p], self.value[p])
        self._graph = None
        self._prog_host = torch.zeros(3, dtype=torch.int64, pin_memory=True)
        self._prog_events = [torch.cuda.Event(), torch.cuda.Event()]
        self.rounds = self.replays = self.eager_rounds = 0          # of the last run()

    def _stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def round(self):
        stream = self._stream()
        L = _eng.lib()
        for p in (0, 1):
            self.engines[p].tick(self.policy[p].data_ptr(), self.value[p].data_ptr(), self.planes[p].data_ptr(), stream)
            pr, va = self.pvs[p](self.planes[p])
            if pr.data_ptr() != self.policy[p].data_ptr():
                self.policy[p].copy_(pr.reshape(self.G, self.C))
            if va.data_ptr() != self.value[p].data_ptr():
                self.value[p].copy_(va.reshape(self.G))
            _eng._check(L.af_match_step(self._match, stream), "af_match_step")
        self.rounds += 1

    def _post_progress(self):
        _eng._check(_eng.lib().af_match_progress_async(self._match, self._stream(), self._prog_host.data_ptr()), "af_match_progress_async")

    def _graph_key(self, rounds_per_replay):
        return (int(rounds_per_replay), self.engines[0].params_key(), self.engines[1].params_key(),
                tuple(v() if v is not None else None for v in self._versions))

    def _raise_first_error(self, code):
        raise _eng.EngineError("device arena: a game failed: %s (code %d)" % (_eng.lib().af_strerror(code).decode(), code))

    def run(self, n_games=None, max_plies=None, rounds_per_replay=8, graph=True):
        """Play n_games (default: all G slots) games of at most max_plies plies (default: until the board is full) ->
        the dict of play_matches.  graph=True: one eager round (weight pack, lazy allocations: the protocol of
        SelfPlayEngine.run_ticks_graph), then rounds_per_replay rounds + the progress copy captured as one graph — keyed on
        rounds_per_replay, both engines' params_key() and both evaluators' weight versions, kept across run() calls — and replayed
        until the progress word read after the PREVIOUS replay's event says every game is over, stopped or failed.  A failing
        capture raises.  graph=False: the same rounds, launched one by one.  Either way the loop is bounded: more than
        max_plies * (2 * upper_simulation_per_step + TICK_SLACK) rounds (a tick parks a simulation on a leaf or yields after a
        budget of selects, and a move has at most upper simulations) raise EngineError."""
        torch = self.torch
        n_games = self.G if n_games is None else int(n_games)
        limit = int(max_plies or self.C)
        if graph and self._version_missing:
            raise _eng.EngineError("DeviceArena.run(graph=True): an evaluator takes bind_outputs but exposes no weights_version (a "
                                   "replayed graph would keep evaluating with stale weights); pass weights_versions=")
        stream = self._stream()
        _eng._check(_eng.lib().af_match_start(self._match, stream, n_games, limit), "af_match_start")
        self.rounds = self.replays = self.eager_rounds = 0
        self._prog_host.zero_()
        bound = limit * (2 * int(self.cfg.upper_simulation_per_step) + TICK_SLACK)
        n = int(rounds_per_replay)
        turn, posted = 0, 0
        if graph and (self._graph is None or self._graph[0] != self._graph_key(n)):
            self._graph = None
            self.round()                             # outside the capture: weight reload, lazy allocations, side-stream creation
            self.eager_rounds += 1
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                for _ in range(n):
                    self.round()
                self._post_progress()
            self.rounds -= n                         # (capture recorded the launches, it did not run them)
            self._graph = (self._graph_key(n), g)
        while True:
            if self.rounds > bound:
                raise _eng.EngineError("device arena: %d games not finished after %d rounds (bound %d)" % (n_games, self.rounds, bound))
            if graph:
                self._graph[1].replay()
                self.rounds += n
                self.replays += 1
            else:
                for _ in range(n):
                    self.round()
                self.eager_rounds += n
                self._post_progress()
            turn ^= 1
            self._prog_events[turn].record(torch.cuda.current_stream(self.dev))
            posted += 1
            if posted < 2:
                continue
            self._prog_events[turn ^ 1].synchronize()            # the previous batch of rounds: the newest keeps the device busy
            done, _, err = (int(x) for x in self._prog_host)
            if err:
                torch.cuda.synchronize(self.dev)
                self._raise_first_error(err)
            if done >= n_games:
                break
        return self.results(n_games)

    def results(self, n_games=None):
        n_games = self.G if n_games is None else int(n_games)
        res, lens = np.zeros(self.G, np.int32), np.zeros(self.G, np.int32)
        mv = np.zeros((self.G, self.C), np.int32)
        rc = _eng.lib().af_match_results(self._match, self._stream(), _eng._p(res, ctypes.c_int32), _eng._p(lens, ctypes.c_int32),
                                         _eng._p(mv, ctypes.c_int32))
        if rc < 0:
            self._raise_first_error(rc)
        res, lens = res[:n_games], lens[:n_games]
        return dict(wins=[int((res == MATCH_WIN0).sum()), int((res == MATCH_WIN1).sum())], draws=int((res == MATCH_DRAW).sum()),
                    moves=[[int(c) for c in mv[i, :lens[i]]] for i in range(n_games)], lengths=[int(x) for x in lens])

    def close(self):
        if getattr(self, "_match", None):
            _eng.lib().af_match_destroy(self._match)             # before its engines
            self._match = None
        for e in getattr(self, "engines", []):
            e.close()

    __del__ = close


def play_matches_device(cfg, pv0, pv1, n_games, device=0, seed0=0, seed1=1, node_cap=0, max_plies=None, **run_kw):
    """play_matches on a DeviceArena: same arguments, same dict, the same games to the cell.  run_kw: rounds_per_replay, graph."""
    a = DeviceArena(cfg, pv0, pv1, n_games, device=device, seed0=seed0, seed1=seed1, node_cap=node_cap)
    try:
        return a.run(n_games, max_plies=max_plies, **run_kw)
    finally:
        a.close()


def ladder(cfg, ckpt_paths, games, match_fn=None, result_path=None, log=print, net_factory=None):
    """The bracket of choose_best_player.py:37-85 over checkpoints ordered oldest to newest: low, high = 0, len - 1; while low < high
    ckpt[low] (player 0) plays ckpt[high] (player 1) `games` games; wins0 < wins1 drops the low one (low += 1, player 0 takes the next
    checkpoint), anything else — a tie included — drops the high one (high -= 1, player 1 takes the previous one).  After every
    pairing the reference's line "<ckpt0>: <ckpt1> = <w0>: <w1>" is appended to result_path (:84), if given.
    -> [(ckpt0, ckpt1, w0, w1, draws)] in the order played.

    match_fn(path0, path1, games) -> (w0, w1, draws).  Default: one DeviceArena of `games` slots, reused across the pairings, over
    two ResNets on the hip backend whose weights are swapped with ResNet.restore (a ".npz" path: load_npz / set_variables).
    net_factory: what the default match_fn builds its two nets with instead of ResNet(cfg.board_size) — for a bracket over deep
    checkpoints, lambda: DeepResNet(S, blocks, 128); its .npz files are loaded in place into the nets' evaluators.
    Not reproduced: the reference plays the games of a pairing one after the other and breaks off after 30 of them at a 2:1 score
    (:65-72); a batch of simultaneous games has no "after 30 games", so every pairing plays all its games."""
    paths = list(ckpt_paths)
    own = None
    if match_fn is None:
        own = match_fn = _arena_match_fn(cfg, games, net_factory=net_factory)
    out = []
    low, high = 0, len(paths) - 1
    try:
        while low < high:
            c0, c1 = paths[low], paths[high]
            w0, w1, draws = match_fn(c0, c1, games)
            line = "%s: %s = %d: %d" % (c0, c1, w0, w1)
            if log is not None:
                log(line)
            if result_path is not None:
                with open(result_path, "a") as f:
                    f.write(line + "\n")
            out.append((c0, c1, int(w0), int(w1), int(draws)))
            if w0 < w1:
                low += 1
            else:
                high -= 1
    finally:
        if own is not None:
            own.close()
    return out


def _arena_match_fn(cfg, games, device=0, net_factory=None):
    """ladder's default match_fn: the nets and the arena are built at the first pairing and kept.  net_factory() -> a net; a
    DeepResNet plays through an evaluator of its own for `games` slots, a ResNet through select_backend("hip")."""
    state = {}

    def load(net, path):
        if str(path).endswith(".npz"):
            net.load_npz(path)
        else:
            net.restore(path)

    def match(path0, path1, n):
        from .network import ResNet
        from .network_deep import DeepResNet
        if not state:
            make = net_factory or (lambda: ResNet(cfg.board_size, device="cuda:%d" % device))
            state["nets"] = [make() for _ in range(2)]
            state["loaded"] = [None, None]
            pvs = [net.evaluator(n) if isinstance(net, DeepResNet) else net.select_backend("hip") for net in state["nets"]]
            state["arena"] = DeviceArena(cfg, pvs[0], pvs[1], n, device=device)
        for p, path in enumerate((path0, path1)):
            if state["loaded"][p] != path:               # the bracket moves one end at a time: the other net keeps its weights
                load(state["nets"][p], path)
                state["loaded"][p] = path
        r = state["arena"].run(n)
        return r["wins"][0], r["wins"][1], r["draws"]

    def close():
        if state:
            state["arena"].close()
            for pv in state["arena"].pvs:
                pv.close()
            state.clear()

    match.close = close
    return match
