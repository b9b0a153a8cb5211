"""arena.ladder: the bracket of the reference's choose_best_player.py:37-85, with the matches injected (no GPU)."""
from conftest import make_cfg


def test_ladder_follows_the_reference_bracket(tmp_path):
    from alphafive_amd import arena
    ckpts = ["ckpt-%d" % i for i in range(5)]
    # (player 0, player 1) -> (wins0, wins1, draws)
    table = {("ckpt-0", "ckpt-4"): (3, 7, 0),      # 0 loses: low -> 1
             ("ckpt-1", "ckpt-4"): (6, 3, 1),      # 4 loses: high -> 3
             ("ckpt-1", "ckpt-3"): (4, 4, 2),      # a tie moves high -> 2
             ("ckpt-1", "ckpt-2"): (2, 5, 3)}      # 1 loses: low -> 2 = high: done
    calls = []

    def match_fn(p0, p1, games):
        calls.append((p0, p1, games))
        return table[(p0, p1)]

    path = tmp_path / "result.txt"
    logged = []
    out = arena.ladder(make_cfg(), ckpts, 10, match_fn=match_fn, result_path=str(path), log=logged.append)
    assert calls == [("ckpt-0", "ckpt-4", 10), ("ckpt-1", "ckpt-4", 10), ("ckpt-1", "ckpt-3", 10), ("ckpt-1", "ckpt-2", 10)]
    assert out == [("ckpt-0", "ckpt-4", 3, 7, 0), ("ckpt-1", "ckpt-4", 6, 3, 1), ("ckpt-1", "ckpt-3", 4, 4, 2), ("ckpt-1", "ckpt-2", 2, 5, 3)]
    lines = path.read_text().splitlines()
    assert lines == ["ckpt-0: ckpt-4 = 3: 7", "ckpt-1: ckpt-4 = 6: 3", "ckpt-1: ckpt-3 = 4: 4", "ckpt-1: ckpt-2 = 2: 5"]
    assert logged == lines


def test_ladder_degenerate_brackets(tmp_path):
    from alphafive_amd import arena

    def never(*a):
        raise AssertionError("no pairing to play")

    assert arena.ladder(make_cfg(), ["only"], 4, match_fn=never, log=None) == []
    assert arena.ladder(make_cfg(), [], 4, match_fn=never, log=None) == []
    # player 0 always wins: high walks down to low, player 0 never changes; no result file unless asked for
    out = arena.ladder(make_cfg(), ["a", "b", "c"], 4, match_fn=lambda p0, p1, n: (n, 0, 0), log=None)
    assert [(r[0], r[1]) for r in out] == [("a", "c"), ("a", "b")]
    assert list(tmp_path.iterdir()) == []
