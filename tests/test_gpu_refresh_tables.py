"""Opt-in refresh tables ("finny tables": RefreshTable, src/eval/nnue/input.h:308-328; refreshPsqAccumulator,
src/eval/nnue_state.cpp:458-524) on the incremental path: spx_acc_reserve_refresh_tables / spx_acc_bind_refresh_tables.
A perspective whose king changed bucket or mirror half is rebuilt from the table cell bound to its parent slot instead of from
scratch. Results never depend on what the tables hold - every evaluation here must equal a full refresh, the reference's
incremental values or the CPU oracle, and the counters must show the tables at work."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NO_TABLE = 0xFFFFFFFF
KERNEL_PATH = {"update_chain_max": 0}  # every batch through spx_update_kernel + the rebuild pass (where tables are consulted)


def preset_of(path):
    import gzip

    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        return f.readline().split()[2].rstrip(";")


def king_bucket(sq_rel):  # spx_device_math.h kingBucket (arch.h:53-65, psq.h:209-226)
    rank, file = sq_rel >> 3, sq_rel & 7
    i = rank * 4 + min(file, 7 - file)
    return int(((0xBA98BA9876543210 if i < 16 else 0xFFEEFFEEDDCCDDCC) >> ((i & 15) * 4)) & 0xF)


def refresh_entry(colour, king_sq):  # getRefreshTableEntry (psq.h:256-262); colour 1 = white
    return king_bucket(king_sq ^ 56 if colour == 0 else king_sq) * 2 + (1 if (king_sq & 7) >= 4 else 0)


def king_square(sp, rec, colour):
    mail, _ = sp.positions_to_mailboxes(rec[None])
    return int(np.nonzero(mail[0] == (10 | colour))[0][0])


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "trace_*.txt")) +
                                        glob.glob(os.path.join(GOLDEN, "trace_*.txt.gz"))), ids=os.path.basename)
def test_trace_replay_with_one_table_matches_reference(sp, net_blob, path):
    """Every reference trace (the two 64k ones included) replayed level by level with every slot bound to ONE table."""
    from stormphrax_amd.trace import Trace, replay

    trace = Trace(path)
    with sp.NnueState(sp.Network(net_blob(preset_of(path))), device=0, max_batch=4096, options=KERNEL_PATH) as st:
        st.reserve_slots(trace.n_nodes)
        st.reserve_refresh_tables(1)
        st.bind_refresh_tables(np.arange(trace.n_nodes, dtype=np.uint32), np.zeros(trace.n_nodes, dtype=np.uint32))
        got, ref_inc, _ = replay(st, trace)
        stats = st.refresh_table_stats()
    bad = np.nonzero(got != ref_inc)[0]
    assert bad.size == 0, f"{bad.size} of {len(got)} EVALs differ; first at eval #{bad[0]}: got {got[bad[0]]} want {ref_inc[bad[0]]}"
    assert stats["served"] > 0 and stats["rebuilt"] >= stats["served"], stats


def _walk(sp, st, start, plies, seed):
    """Forward-and-back walk of len(start) games: every ply one random move per game (materialising update, ping-pong
    slots) and, from the same parents, a second random move evaluated eval-only; every third ply steps back to the
    grandparent's board (an unmake is a one-move delta too). Returns the evaluations of every ply."""
    games = len(start)
    slots = [np.arange(games, dtype=np.uint32), np.arange(games, 2 * games, dtype=np.uint32)]
    st.reset(start, slots[0])
    history = [start]
    outs = []
    for ply in range(plies):
        cur = history[-1]
        if ply % 3 == 2 and len(history) >= 2:
            nxt = history[-2]
        else:
            nxt = sp.random_successors(cur, seed=seed + ply)[0]
        side = sp.random_successors(cur, seed=seed + 5000 + ply)[0]
        outs.append(st.update_evaluate(slots[ply & 1], None, side))
        outs.append(st.update_evaluate(slots[ply & 1], slots[(ply + 1) & 1], nxt))
        history.append(nxt)
        outs.append((side, nxt))
    return outs


@pytest.mark.parametrize("preset", ["tame", "wild", "extreme", "realistic", "mixed", "near"])
def test_table_contents_never_matter(sp, net_blob, preset):
    """4 096 games x 40 plies on three contexts - no tables, fresh tables (one per game), and tables primed with unrelated
    DFRC games under a random game -> table map where several games share a table - give identical evaluations, equal to
    evaluate_once of the boards (u8, i16 and near-compact piece-square rows, the i16 wrap of `extreme`)."""
    games, plies = 4096, 40
    start = sp.random_positions(games, seed=71, min_ply=0, max_ply=60, dfrc_every=3)
    blob = net_blob(preset)
    results, served = [], []
    for mode in ("none", "fresh", "primed"):
        with sp.NnueState(sp.Network(blob), device=0, max_batch=games, options=KERNEL_PATH) as st:
            st.reserve_slots(2 * games)
            if mode == "fresh":
                st.reserve_refresh_tables(games)
                g = np.arange(games, dtype=np.uint32)
                st.bind_refresh_tables(np.concatenate([g, g + games]), np.concatenate([g, g]))
            elif mode == "primed":
                n_tables = games // 4
                st.reserve_refresh_tables(n_tables)
                # prime every table with unrelated DFRC games first
                st.bind_refresh_tables(np.arange(2 * games, dtype=np.uint32), np.arange(2 * games, dtype=np.uint32) % n_tables)
                _walk(sp, st, sp.random_positions(games, seed=99, min_ply=0, max_ply=20, dfrc_every=1), 12, 900)
                st.refresh_table_stats()
                table_of = np.random.default_rng(5).integers(0, n_tables, size=games).astype(np.uint32)
                g = np.arange(games, dtype=np.uint32)
                st.bind_refresh_tables(np.concatenate([g, g + games]), np.concatenate([table_of, table_of]))
            outs = _walk(sp, st, start, plies, 300)
            served.append(st.refresh_table_stats()["served"])
            if mode == "none":
                for k in range(0, len(outs), 3):
                    side, nxt = outs[k + 2]
                    assert np.array_equal(outs[k], st.evaluate_once(side)), f"ply {k // 3}: eval-only children"
                    assert np.array_equal(outs[k + 1], st.evaluate_once(nxt)), f"ply {k // 3}: materialised children"
            results.append([o for i, o in enumerate(outs) if i % 3 != 2])
    for k in range(len(results[0])):
        assert np.array_equal(results[0][k], results[1][k]), f"fresh tables differ at output {k}"
        assert np.array_equal(results[0][k], results[2][k]), f"primed tables differ at output {k}"
    assert served[0] == 0 and served[1] > 0 and served[2] > 0, served


def test_sibling_collision_one_writer_per_cell(sp, net_blob, oracle):
    """A parent whose king has several legal moves into the same (bucket, mirror half): all its children evaluated eval-only
    in ONE batch with the parent bound. The table serves exactly one perspective per distinct (table, entry, colour) cell
    among the deferred ones; the others rebuild from scratch; every value equals evaluate_once and the oracle."""
    blob = net_blob("wild")
    parent = sp.positions_from_fens(["4k3/pp4pp/8/8/4K3/8/PP4PP/8 w - - 0 1"])
    mg_children = None
    with sp.NnueState(sp.Network(blob), device=0, max_batch=256, options=KERNEL_PATH) as st:
        mg = st.movegen(parent)
        n = int(mg["count"][0])
        mg_children = mg["children"][:n]
        st.reserve_slots(1)
        st.reset(parent, np.zeros(1, dtype=np.uint32))
        st.reserve_refresh_tables(1)
        st.bind_refresh_tables(np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32))
        got = st.update_evaluate(np.zeros(n, dtype=np.uint32), None, mg_children)
        stats = st.refresh_table_stats()
        assert np.array_equal(got, st.evaluate_once(mg_children))
    oracle.use(blob, "wild")
    mail, stm = sp.positions_to_mailboxes(mg_children)
    assert np.array_equal(got, oracle.eval_mailboxes(mail, stm))
    cells, deferred = set(), 0
    for c in (0, 1):
        kp = king_square(sp, parent[0], c)
        for child in mg_children:
            kc = king_square(sp, child, c)
            if refresh_entry(c, kp) != refresh_entry(c, kc):
                deferred += 1
                cells.add((refresh_entry(c, kc), c))
    assert deferred > len(cells) >= 2, (deferred, cells)  # siblings do collide in this position
    assert stats["rebuilt"] == deferred and stats["served"] == len(cells), (stats, deferred, cells)


def test_every_update_path_and_the_bindings(sp, net_blob):
    """Materialising, eval-only, counted and pipelined (async) plies with tables equal full refreshes; arena growth keeps the
    bindings; argument errors; unbound slots behave as on a context without tables."""
    import ctypes

    from stormphrax_amd import _lib

    lib = _lib.load()
    games, plies = 4096, 8
    chain = [sp.random_positions(games, seed=13, min_ply=0, max_ply=80, dfrc_every=3)]
    for ply in range(plies):
        chain.append(sp.random_successors(chain[-1], seed=400 + ply)[0])
    with sp.NnueState(sp.Network(net_blob("realistic")), device=0, max_batch=games, options=KERNEL_PATH) as st:
        st.reserve_slots(2 * games)
        st.reserve_refresh_tables(16)
        # argument errors
        for slots, tables in (([2 * games], [0]), ([0], [16]), ([0, 2 * games + 5], [1, 1])):
            with pytest.raises(_lib.SpxError) as err:
                st.bind_refresh_tables(slots, tables)
            assert err.value.code == 1
        assert lib.spx_acc_reserve_refresh_tables(None, 1) == 1
        assert lib.spx_acc_bind_refresh_tables(st._h, None, None, 1) == 1
        st.bind_refresh_tables([0], [NO_TABLE])  # unbinding is valid
        # unbound slots: the tables exist but nothing consults them
        slots = [np.arange(games, dtype=np.uint32), np.arange(games, 2 * games, dtype=np.uint32)]
        st.reset(chain[0], slots[0])
        st.update(slots[0], slots[1], chain[1])
        assert np.array_equal(st.evaluate(slots[1]), st.evaluate_once(chain[1]))
        assert st.refresh_table_stats()["served"] == 0
        # bind every game's slots (games share the 16 tables), then grow the arena: the bindings survive
        g = np.arange(games, dtype=np.uint32)
        st.bind_refresh_tables(np.concatenate([g, g + games]), np.concatenate([g % 16, g % 16]))
        st.reserve_slots(2 * games + 100)
        st.reset(chain[1], slots[1])
        st.update(slots[1], slots[0], chain[2])                                     # materialising
        assert np.array_equal(st.evaluate(slots[0]), st.evaluate_once(chain[2]))
        assert np.array_equal(st.update_evaluate(slots[0], None, chain[3]), st.evaluate_once(chain[3]))  # eval-only
        assert st.refresh_table_stats()["served"] > 0
        # counted (device-resident record count) and pipelined plies; buffers in page-locked, device-mapped host memory
        ptrs = []

        def pinned(array):
            raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
            p = lib.spx_host_alloc(raw.size)
            assert p
            ptrs.append(p)
            view = np.ctypeslib.as_array((ctypes.c_uint8 * raw.size).from_address(p))
            view[:] = raw
            return p, view

        try:
            d_slots = [pinned(s)[0] for s in slots]
            d_boards = [pinned(c)[0] for c in chain]
            d_count = pinned(np.array([games - 7], dtype=np.uint32))[0]
            outs = [pinned(np.full(games, -1, dtype=np.int32))[1].view(np.int32) for _ in range(3, plies + 1)]
            _lib.check(lib.spx_acc_update_eval_device_counted(st._h, d_slots[0], d_slots[1], d_boards[3], d_count, games,
                                                              outs[0].ctypes.data, None))
            st.synchronize()
            assert np.array_equal(outs[0][: games - 7], st.evaluate_once(chain[3][: games - 7]))
            st.update(slots[0], slots[1], chain[3])  # (the last 7 records were not updated by the counted call)
            for k, ply in enumerate(range(4, plies + 1), start=1):
                _lib.check(lib.spx_acc_update_eval_device_async(st._h, d_slots[(ply + 1) & 1], d_slots[ply & 1], d_boards[ply],
                                                                games, outs[k].ctypes.data, None))
            st.synchronize()
            for k, ply in enumerate(range(4, plies + 1), start=1):
                assert np.array_equal(outs[k], st.evaluate_once(chain[ply])), f"pipelined ply {ply}"
        finally:
            for p in ptrs:
                lib.spx_host_free(p)
        assert st.refresh_table_stats()["served"] > 0


def _games(data):
    """The viriformat games of a file (32-byte start record, then 4-byte move words up to a zero word), sorted."""
    out, i = [], 0
    while i < len(data):
        j = i + 32
        while data[j:j + 4] != b"\0\0\0\0":
            j += 4
        out.append(data[i:j + 4])
        i = j + 4
    assert out
    return sorted(out)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("nodes", [0, 64])
def test_selfplay_with_refresh_tables_is_byte_identical(sp, net_blob, tmp_path, graph, nodes):
    """Same seed with and without SPX_SELFPLAY_REFRESH_TABLES (depth-1 and a 64-node search, direct launches and graphs): the
    same games byte for byte, and the tables serve rebuilds. The host move generation path refuses the flag. (Games are
    compared as a sorted list: the order in which the two halves' seats append finished games to the file varies from run
    to run with or without tables - the games themselves do not.)"""
    from stormphrax_amd import _lib

    files, served = [], []
    for tables in (False, True):
        with sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=64 * 96,
                          options={"selfplay_graph": graph}) as st:
            path = str(tmp_path / f"sp_{int(tables)}.vf")
            stats = st.selfplay(n_games=64, target_games=96, out_path=path, max_plies=80, dfrc=True, temperature_cp=20,
                                seed=17, search_nodes=nodes, refresh_tables=tables)
            assert stats["games"] == 96
            served.append(st.refresh_table_stats()["served"])
            files.append(open(path, "rb").read())
            if tables and graph == 0 and nodes == 0:
                with pytest.raises(_lib.SpxError) as err:
                    st.selfplay(n_games=4, target_games=4, max_plies=20, host_movegen=True, refresh_tables=True)
                assert err.value.code == 1
    assert _games(files[0]) == _games(files[1])
    assert served[0] == 0 and served[1] > 0, served
