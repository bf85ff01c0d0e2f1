"""Pruned quiescence in the live self-play search (SPX_SELFPLAY_QUIESCE_PRUNING): the games against the recursive restatement
of tests/_qprune_rules.py (itself checked on the CPU by tests/test_qprune_rules.py, whose last test showed on the 16 fixed roots
that the grid below takes every branch of the node, plays moves the unpruned search would not and expands fewer nodes in sum)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = [(25, 1, 8, 10, 30, 1, True), (25, 4, 4, 4, 20, 0, False), (25, 8, 2, 2, 12, 1, False),
        (150, 1, 3, 3, 20, 0, False), (150, 4, 2, 2, 14, 1, False), (150, 8, 2, 2, 10, 0, False)]


def play_and_verify(sp, st, oracle, net_blob, path, budget, q, n_games, target, max_plies, dfrc, seed, preset="tame", compare=True):
    """One pruned-quiescence run replayed through the restatement -> (stats, the searcher, per ply whether the unpruned
    quiescence search would have played another move, that unpruned searcher)."""
    from _qprune_rules import verify_qprune_file

    stats = st.selfplay(n_games=n_games, target_games=target, out_path=path, max_plies=max_plies, dfrc=dfrc, temperature_cp=0,
                        seed=seed, search_nodes=budget, quiesce_plies=q, quiesce_pruning=True)
    assert stats["games"] == target and sum(stats["outcomes"]) == target
    oracle.use(net_blob(preset), preset)
    tally, plain = {}, [] if compare else None
    checked, searcher, deepest, unpruned = verify_qprune_file(sp, st, oracle, open(path, "rb").read(), max_plies, budget, q, tally,
                                                              plain)
    assert checked == stats["positions"] == searcher.searches
    per_search = max(budget, searcher.largest_search)
    assert searcher.expanded <= stats["steps"] <= searcher.expanded + 4 * (target + n_games) * per_search
    print(f"budget {budget} Q {q}: {checked} plies, {searcher.expanded} nodes restated ({searcher.quiesce_nodes} quiescence; "
          f"{stats['steps']} expanded by the driver, {stats['evals']} leaves), deepest iteration {deepest}, deepest quiescence ply "
          f"{searcher.deepest_quiesce}, candidates {searcher.candidates} of {searcher.legal} legal moves; {searcher.taken}; "
          + (f"{sum(plain)}/{len(plain)} moves differ from the unpruned search, which expanded {unpruned.quiesce_nodes} quiescence "
             f"nodes on the same roots; " if compare else "") + f"{tally}")
    return stats, searcher, plain, unpruned


@pytest.fixture(scope="module")
def played(sp, net_blob, oracle, tmp_path_factory):
    """case of GRID -> (searcher, per-ply "the unpruned search plays another move", the unpruned searcher): every case is played and
    replayed once per session, whichever test asks first - so the test that sums over the grid does not depend on the others
    having run, on their order or on their process."""
    done = {}

    def play(case):
        if case not in done:
            budget, q, n_games, target, max_plies, graph, dfrc = case
            state = sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=16384, options={"selfplay_graph": graph})
            try:
                path = str(tmp_path_factory.mktemp("qprune") / "q.vf")
                _, searcher, plain, unpruned = play_and_verify(sp, state, oracle, net_blob, path, budget, q, n_games, target,
                                                               max_plies, dfrc, seed=budget + q)
            finally:
                state.close()
            done[case] = (searcher, plain, unpruned)
        return done[case]

    return play


@pytest.mark.parametrize("case", GRID, ids=lambda c: "budget%d-q%d-graph%d" % (c[0], c[1], c[5]))
def test_pruned_quiescence_games_follow_the_restated_search(played, case):
    """Every recorded game through tests/_qprune_rules.py: the move at every ply, the scores, lengths and outcomes, a sample of the
    leaves against the CPU oracle, stats.steps against the restatement's expansion count (play_and_verify asserts them). The
    non-vacuity conditions are summed over the grid by the test below."""
    searcher, plain, _ = played(case)
    assert searcher.quiesce_nodes > 0 and len(plain) == searcher.searches


def test_the_grid_exercised_every_branch(played):
    """Over the whole grid (cases not played yet are played here): every branch of the node taken at least once, a move the
    unpruned quiescence search would not have played, fewer quiescence nodes in sum than the unpruned restatement on the same
    roots."""
    taken, differ, pruned_nodes, unpruned_nodes = {}, 0, 0, 0
    for case in GRID:
        searcher, plain, unpruned = played(case)
        for name, n in searcher.taken.items():
            taken[name] = taken.get(name, 0) + n
        differ += sum(plain)
        pruned_nodes += searcher.quiesce_nodes
        unpruned_nodes += unpruned.quiesce_nodes
    print({"taken": taken, "differ": differ, "pruned nodes": pruned_nodes, "unpruned nodes": unpruned_nodes})
    assert all(n > 0 for n in taken.values()), taken
    assert differ >= 1
    assert pruned_nodes < unpruned_nodes


def test_refresh_tables_play_the_same_files_with_pruning(sp, net_blob, tmp_path):
    from _datagen_rules import parse_games

    def play(name, n_games, target, **kw):
        with sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=16384) as state:
            path = str(tmp_path / name)
            stats = state.selfplay(n_games=n_games, target_games=target, out_path=path, max_plies=40, dfrc=True, temperature_cp=0,
                                   seed=5, **kw)
            assert stats["games"] == target
            return open(path, "rb").read(), stats

    unpruned, _ = play("u.vf", 1, 2, search_nodes=30, quiesce_plies=4)
    sets = []
    for tables in (False, True):
        one, s1 = play(f"one{int(tables)}.vf", 1, 2, search_nodes=30, quiesce_plies=4, quiesce_pruning=True, refresh_tables=tables)
        many, _ = play(f"many{int(tables)}.vf", 12, 20, search_nodes=30, quiesce_plies=4, quiesce_pruning=True, refresh_tables=tables)
        sets.append((one, s1["steps"], s1["evals"], sorted((h, m.tobytes(), s.tobytes()) for h, m, s, _ in parse_games(many))))
    assert sets[0] == sets[1] and len(sets[0][3]) == 20
    assert sets[0][0] != unpruned   # and pruning does play other games than the unpruned quiescence search


def test_two_member_group_with_pruning_verifies(sp, net_blob, oracle, tmp_path):
    from _qprune_rules import verify_qprune_file

    net = sp.Network(net_blob("tame"))
    with sp.DeviceGroup(net, devices=[0, 0], max_batch_per_device=4096) as grp:
        stats = grp.selfplay(n_games=4, target_games=6, out_path=str(tmp_path / "g"), max_plies=16, dfrc=True, temperature_cp=0,
                             seed=2, search_nodes=20, quiesce_plies=2, quiesce_pruning=True)
        assert stats["games"] == 6 and stats["steps"] >= stats["positions"]
    oracle.use(net_blob("tame"), "tame")
    with sp.NnueState(net, device=0, max_batch=4096) as state:
        checked, expanded = 0, []
        for r in (0, 1):
            n, searcher, _, _ = verify_qprune_file(sp, state, oracle, open(str(tmp_path / f"g.{r}.vf"), "rb").read(), 16, 20, 2)
            checked += n
            expanded.append(searcher.expanded)
            assert searcher.quiesce_nodes > 0
        assert checked == stats["positions"] and max(expanded) <= stats["steps"]


def test_pruning_argument_checks(sp, net_blob):
    """The flag needs quiescence plies, hence also the search proper (k >= 2) and the device-resident driver."""
    from stormphrax_amd import _lib

    with sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=4096) as state:
        for kw in ({"search_nodes": 8, "quiesce_plies": 0}, {"search_nodes": 0, "quiesce_plies": 0},
                   {"search_nodes": 1, "quiesce_plies": 2}, {"search_nodes": 0, "quiesce_plies": 2},
                   {"search_nodes": 8, "quiesce_plies": 2, "host_movegen": True}, {"host_movegen": True}):
            with pytest.raises(_lib.SpxError) as err:
                state.selfplay(n_games=4, target_games=4, max_plies=20, quiesce_pruning=True, **kw)
            assert err.value.code == 1, kw   # SPX_ERR_INVALID_ARG
        assert state.selfplay(n_games=4, target_games=4, max_plies=20, search_nodes=2, quiesce_plies=8, quiesce_pruning=True)["games"] == 4


@pytest.mark.parametrize("n_games,target,budget,q", [(1, 1, 7, 2), (1, 3, 30, 1), (5, 2, 12, 3), (33, 40, 3, 2)])
def test_pruning_edge_sizes(sp, net_blob, oracle, tmp_path, n_games, target, budget, q):
    """One seat, fewer games than seats, more games than seats, tiny budgets: exactly `target` games, every one of them following
    the restated search."""
    with sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=4096) as state:
        play_and_verify(sp, state, oracle, net_blob, str(tmp_path / "edge.vf"), budget, q, n_games, target, 16, False, seed=11,
                        compare=False)
