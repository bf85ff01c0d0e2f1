"""Quiescence search in the live self-play search (SPX_SELFPLAY_QUIESCE_PLIES) and the move generator's quiescence mode
(spx_movegen_modes): the generator against the host chess core filtered by the Python predicate of tests/_qsearch_rules.py,
the games against the recursive restatement there (itself checked on the CPU by tests/test_qsearch_rules.py)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

QUIESCE_FENS = [
    "1n2k3/P7/8/8/8/8/8/R3K2R w KQ - 0 1",                                        # quiet + capturing promotion, both castlings
    "r3k2r/8/8/8/8/8/p7/1N2K3 b kq - 0 1",                                        # the same for black, on the other wing's file
    "n1n5/PPPk4/8/8/8/8/4Kppp/5N1N b - - 0 1", "n1n5/PPPk4/8/8/8/8/4Kppp/5N1N w - - 0 1",
    "4k2n/6P1/8/8/8/8/1p6/N3K3 w - - 0 1", "4k2n/6P1/8/8/8/8/1p6/N3K3 b - - 0 1",  # promotions on both wings
    "rnbqkb1r/ppp1pppp/5n2/3pP3/8/8/PPPP1PPP/RNBQKBNR w KQkq d6 0 3", "4k3/8/8/8/3pP3/8/8/4K3 b - e3 0 1",  # en passant
    "8/8/8/8/k2Pp2Q/8/8/3K4 b - d3 0 1",                                          # en passant would expose the king
    "4k3/8/8/8/8/8/4r3/4K3 w - - 0 1", "4k3/8/8/8/8/2n5/3b4/4K3 w - - 0 1",        # in check: every evasion
    "4k3/4r3/8/8/8/8/3p4/4K3 w - - 0 1",                                          # in check by a pawn about to promote
    "R6k/6pp/8/8/8/8/8/4K3 b - - 0 1", "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1",           # mate, stalemate
    "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
    "bqnb1rkr/pp3ppp/3ppn2/2p5/5P2/P2P4/NPP1P1PP/BQ1BNRKR w HFhf - 2 9", "rk5r/8/8/8/8/8/8/RK5R w HAha - 0 1",
    "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1",
]


@pytest.fixture(scope="module")
def st(sp, net_blob):
    s = sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=16384)
    yield s
    s.close()


def generator_positions(sp):
    fens = [json.loads(line)["fen"] for line in open(os.path.join(GOLDEN, "evals.jsonl"))]
    return np.concatenate([
        sp.positions_from_fens(QUIESCE_FENS), sp.positions_from_fens(fens),
        sp.random_positions(2500, seed=41, min_ply=0, max_ply=200, dfrc_every=2),
        sp.random_positions(800, seed=42, min_ply=0, max_ply=14, dfrc_every=1),    # castling rights still alive
    ])


def test_quiescence_mode_of_the_generator_matches_the_filtered_host_core(sp, st):
    """Mixed modes over the golden positions, hand-made ones and random playouts (DFRC included): per position the children,
    move words, count and in_check equal the host chess core's legal moves filtered by the Python predicate (all of them in
    check or in mode 0), in the relative order the full generation gives them."""
    from _qsearch_rules import is_noisy

    pos = generator_positions(sp)
    n = len(pos)
    assert n >= 2119 + 3300
    cap = 64 * n + 256
    full = st.movegen(pos, capacity=cap)
    modes = (np.arange(n) % 3 != 0).astype(np.uint8)
    modes[:len(QUIESCE_FENS)] = 1
    out = st.movegen(pos, capacity=cap, modes=modes)
    assert int(out["count"].sum()) == len(out["children"]) < len(full["children"])
    seen = {"in check": 0, "ep": 0, "queen alone": 0, "capturing under-promotion": 0, "castling dropped": 0, "no candidate": 0,
            "mode 0": 0}
    for i in range(n):
        words, kids, chk = sp.legal_moves(pos[i])
        keep = [k for k in range(len(words)) if modes[i] == 0 or chk or is_noisy(pos[i], words[k])]
        want = sorted((int(words[k]), kids[k].tobytes()) for k in keep)
        lo, cnt = int(out["first"][i]), int(out["count"][i])
        got = [(int(m), c.tobytes()) for m, c in zip(out["moves"][lo:lo + cnt], out["children"][lo:lo + cnt])]
        fen = sp.position_to_fen(pos[i])
        assert cnt == len(want) and sorted(got) == want, (fen, int(modes[i]), cnt, len(want))
        assert bool(out["in_check"][i]) == bool(chk) == bool(full["in_check"][i]), fen
        assert np.all(out["parents"][lo:lo + cnt] == i)
        # the relative order of the full generation
        flo, fcnt = int(full["first"][i]), int(full["count"][i])
        assert fcnt == len(words)
        wanted = {w for w, _ in want}
        assert [w for w, _ in got] == [int(m) for m in full["moves"][flo:flo + fcnt] if int(m) in wanted], fen
        if modes[i] == 0:
            seen["mode 0"] += 1
            continue
        kinds = [w >> 14 for w, _ in got]
        seen["in check"] += bool(chk)
        seen["ep"] += 1 in kinds
        seen["no candidate"] += cnt == 0 and len(words) > 0
        seen["castling dropped"] += any(int(w) >> 14 == 2 for w in words) and 2 not in kinds
        occ = int(pos[i]["occupancy"])
        promos = [w for w, _ in got if w >> 14 == 3]
        if not chk:
            seen["queen alone"] += any(not (occ >> ((w >> 6) & 63)) & 1 for w in promos)
            seen["capturing under-promotion"] += any(((w >> 12) & 3) != 3 for w in promos)
            assert all(((w >> 12) & 3) == 3 or (occ >> ((w >> 6) & 63)) & 1 for w in promos), fen
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_mode_zero_and_no_modes_are_the_plain_generator_and_the_device_variant_agrees(sp, st):
    """modes = NULL and modes all zero write what spx_movegen writes, byte for byte (one position per call fixes the placement,
    a batch is compared block by block); spx_movegen_modes_device on resident buffers gives the host variant's blocks
    (tests/_movegen_modes_worker.py, a process of its own: the buffers are torch's, which must initialise its HIP runtime
    before the library is loaded)."""
    import subprocess
    import sys

    pos = generator_positions(sp)[:1500]
    n = len(pos)
    cap = 64 * n + 256

    def blocks(o):
        return [(o["moves"][lo:lo + c].tobytes(), o["children"][lo:lo + c].tobytes(), bool(k))
                for lo, c, k in zip(o["first"].tolist(), o["count"].tolist(), o["in_check"])]

    plain = st.movegen(pos, capacity=cap)
    zero = st.movegen(pos, capacity=cap, modes=np.zeros(n, dtype=np.uint8))
    assert blocks(plain) == blocks(zero)
    for i in (0, 1, 5, 700, n - 1):
        a, b = st.movegen(pos[i:i + 1]), st.movegen(pos[i:i + 1], modes=np.zeros(1, dtype=np.uint8))
        for key in ("children", "moves", "parents", "first", "count", "in_check"):
            assert a[key].tobytes() == b[key].tobytes(), (i, key)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "_movegen_modes_worker.py")], cwd=root, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert "modes device ok" in out.stdout


def test_capacity_overflow_is_still_reported(sp, st):
    from stormphrax_amd import _lib

    pos = sp.random_positions(64, seed=3)
    with pytest.raises(_lib.SpxError) as err:
        st.movegen(pos, capacity=100, modes=np.zeros(64, dtype=np.uint8))
    assert err.value.code == 5   # SPX_ERR_CAPACITY
    with pytest.raises(_lib.SpxError) as err:
        st.movegen(np.concatenate([pos] * 8), capacity=100, modes=np.ones(512, dtype=np.uint8))
    assert err.value.code == 5


def play_and_verify(sp, st, oracle, net_blob, path, budget, q, n_games, target, max_plies, dfrc, seed, preset="tame"):
    """One quiescence run replayed through the restatement -> (stats, the searcher, fraction of moves the plain search would
    not have played)."""
    from _qsearch_rules import verify_qsearch_file

    stats = st.selfplay(n_games=n_games, target_games=target, out_path=path, max_plies=max_plies, dfrc=dfrc, temperature_cp=0,
                        seed=seed, search_nodes=budget, quiesce_plies=q)
    assert stats["games"] == target and sum(stats["outcomes"]) == target
    oracle.use(net_blob(preset), preset)
    tally, plain = {}, []
    checked, searcher, deepest = verify_qsearch_file(sp, st, oracle, open(path, "rb").read(), max_plies, budget, q, tally, plain)
    assert checked == stats["positions"] == searcher.searches
    # the driver also expanded the searches of discarded openings and the roots of positions that turned out terminal: a
    # search is at most the largest one seen plus what a first iteration can overshoot by, bounded here by four times as much
    per_search = max(budget, searcher.largest_search)
    assert searcher.expanded <= stats["steps"] <= searcher.expanded + 4 * (target + n_games) * per_search
    print(f"budget {budget} Q {q}: {checked} plies, {searcher.expanded} nodes restated ({searcher.quiesce_nodes} quiescence; "
          f"{stats['steps']} expanded by the driver, {stats['evals']} leaves), deepest iteration {deepest}, deepest quiescence ply "
          f"{searcher.deepest_quiesce}, {searcher.searches_with_quiesce}/{searcher.searches} searches with quiescence nodes, "
          f"candidates {searcher.candidates} of {searcher.legal} legal moves, {sum(plain)}/{len(plain)} moves differ from the "
          f"plain search; {tally}")
    return stats, searcher, plain


@pytest.mark.parametrize("budget,q,n_games,target,max_plies,graph,dfrc", [
    (25, 1, 8, 10, 30, 1, True), (25, 4, 4, 4, 20, 0, False), (25, 8, 2, 2, 12, 1, False),
    (150, 1, 3, 3, 20, 0, False), (150, 4, 2, 2, 14, 1, False), (150, 8, 2, 2, 10, 0, False)])
def test_quiescence_games_follow_the_restated_search(sp, net_blob, oracle, tmp_path, budget, q, n_games, target, max_plies, graph,
                                                     dfrc):
    """Every recorded game through tests/_qsearch_rules.py: the move at every ply, the scores, lengths and outcomes (through
    tests/_datagen_rules.replay_game), a sample of the leaves against the CPU oracle, stats.steps against the restatement's
    expansion count - and the files do exercise quiescence: quiescence nodes in at least half of the searches, quiescence ply
    min(Q, 2) reached, a move the plain search would not have played."""
    state = sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=16384, options={"selfplay_graph": graph})
    try:
        _, searcher, plain = play_and_verify(sp, state, oracle, net_blob, str(tmp_path / "q.vf"), budget, q, n_games, target,
                                             max_plies, dfrc, seed=budget + q)
        assert 2 * searcher.searches_with_quiesce >= searcher.searches and searcher.quiesce_nodes > 0
        assert searcher.deepest_quiesce >= min(q, 2)
        assert sum(plain) >= 1
    finally:
        state.close()


def test_zero_plies_and_refresh_tables_play_the_same_files(sp, net_blob, tmp_path):
    """SPX_SELFPLAY_QUIESCE_PLIES(0) is the flag left out, byte for byte; refresh tables on / off with Q = 4 play the same
    files (one seat: the order of the games in the file is fixed too)."""
    from _datagen_rules import parse_games

    def play(name, n_games, target, **kw):
        with sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=16384) as state:
            path = str(tmp_path / name)
            stats = state.selfplay(n_games=n_games, target_games=target, out_path=path, max_plies=40, dfrc=True, temperature_cp=0,
                                   seed=5, **kw)
            assert stats["games"] == target
            return open(path, "rb").read(), stats

    a, sa = play("a.vf", 1, 3, search_nodes=30)
    b, sb = play("b.vf", 1, 3, search_nodes=30, quiesce_plies=0)
    assert a == b and (sa["steps"], sa["evals"], sa["positions"]) == (sb["steps"], sb["evals"], sb["positions"])
    sets = []
    for tables in (False, True):
        one, s1 = play(f"one{int(tables)}.vf", 1, 2, search_nodes=30, quiesce_plies=4, refresh_tables=tables)
        many, _ = play(f"many{int(tables)}.vf", 12, 20, search_nodes=30, quiesce_plies=4, refresh_tables=tables)
        sets.append((one, s1["steps"], sorted((h, m.tobytes(), s.tobytes()) for h, m, s, _ in parse_games(many))))
    assert sets[0] == sets[1] and len(sets[0][2]) == 20
    assert sets[0][0] != a[:len(sets[0][0])]   # and quiescence does play other games than the plain search


def test_two_member_group_with_quiescence_verifies(sp, net_blob, oracle, tmp_path):
    from _qsearch_rules import verify_qsearch_file

    net = sp.Network(net_blob("tame"))
    with sp.DeviceGroup(net, devices=[0, 0], max_batch_per_device=4096) as grp:
        stats = grp.selfplay(n_games=4, target_games=6, out_path=str(tmp_path / "g"), max_plies=16, dfrc=True, temperature_cp=0,
                             seed=2, search_nodes=20, quiesce_plies=2)
        assert stats["games"] == 6 and stats["steps"] >= stats["positions"]
    oracle.use(net_blob("tame"), "tame")
    with sp.NnueState(net, device=0, max_batch=4096) as state:
        checked, expanded = 0, []
        for r in (0, 1):
            n, searcher, _ = verify_qsearch_file(sp, state, oracle, open(str(tmp_path / f"g.{r}.vf"), "rb").read(), 16, 20, 2)
            checked += n
            expanded.append(searcher.expanded)
            assert searcher.quiesce_nodes > 0
        # (a group reports the steps of the member that took most)
        assert checked == stats["positions"] and max(expanded) <= stats["steps"]


def test_quiescence_argument_checks(sp, net_blob):
    """Q > 0 needs the search proper (k >= 2) and the device-resident driver; Q is at most 8."""
    from stormphrax_amd import _lib

    with sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=4096) as state:
        for kw in ({"search_nodes": 0, "quiesce_plies": 2}, {"search_nodes": 1, "quiesce_plies": 2},
                   {"search_nodes": 8, "quiesce_plies": 2, "host_movegen": True},
                   *({"search_nodes": 8, "quiesce_plies": q} for q in range(9, 16))):
            with pytest.raises(_lib.SpxError) as err:
                state.selfplay(n_games=4, target_games=4, max_plies=20, **kw)
            assert err.value.code == 1, kw   # SPX_ERR_INVALID_ARG
        assert state.selfplay(n_games=4, target_games=4, max_plies=20, search_nodes=2, quiesce_plies=8)["games"] == 4
        for q in (-1, 16, 17):   # the wrappers do not let a value wrap into the four flag bits
            with pytest.raises(ValueError):
                state.selfplay(n_games=4, target_games=4, max_plies=20, search_nodes=8, quiesce_plies=q)


@pytest.mark.parametrize("n_games,target,budget,q", [(1, 1, 7, 2), (1, 3, 30, 1), (5, 2, 12, 3), (33, 40, 3, 2)])
def test_quiescence_edge_sizes(sp, net_blob, oracle, tmp_path, n_games, target, budget, q):
    """One seat, fewer games than seats, more games than seats, tiny budgets: exactly `target` games, every one of them
    following the restated search."""
    with sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=4096) as state:
        play_and_verify(sp, state, oracle, net_blob, str(tmp_path / "edge.vf"), budget, q, n_games, target, 16, False, seed=11)
