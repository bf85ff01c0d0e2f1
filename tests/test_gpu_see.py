"""Static exchange evaluation on the device (spx_see) and the move generator's SEE modes and outputs (spx_movegen_flags, modes 2 /
3): spx_see against the host chess core and the compiled reference's fixture (tests/golden/see.txt.gz), the generator against the
host core's legal moves filtered and flagged by the PYTHON predicates (tests/_see_rules.py, tests/_qsearch_rules.is_noisy)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "see.txt.gz")

SEE_FENS = [
    "4k3/2p5/8/3pP3/8/8/8/4K3 w - d6 0 1",        # the only noisy move is an en passant that fails see(1)
    "1r2k3/P7/8/8/8/8/8/4K3 w - - 0 1",           # a quiet queen promotion that loses the queen (fails see(-81)), a capturing one
    "4k3/8/8/3Q4/8/8/8/r3K3 w - - 0 1",           # in check: interposing the queen loses it, and is still generated
    "4k3/P7/8/8/8/8/8/4K3 w - - 0 1", "1n1rk3/P7/8/8/8/8/8/4K3 w - - 0 1", "4k3/8/8/8/8/8/8/R3K2R w KQ - 0 1",
    "4k3/8/4p3/3p4/8/8/8/3RR1K1 w - - 0 1", "4k3/3p4/8/8/B7/2Q5/8/6K1 w - - 0 1", "4k3/2b5/3p4/4p3/3P4/2B5/8/4K3 w - - 0 1",
    "4k2q/6b1/8/4p3/3P4/5N2/8/4K3 w - - 0 1", "3rk3/3r4/8/3p4/8/8/3R4/3RK3 w - - 0 1", "3rk3/3q4/8/3p4/8/8/3R4/3QK3 w - - 0 1",
    "4k3/8/8/8/8/1n6/3r4/3RK3 w - - 0 1", "4k3/8/8/b7/8/1n6/3r4/3RK3 w - - 0 1",
]


@pytest.fixture(scope="module")
def st(sp, net_blob):
    s = sp.NnueState(sp.Network(net_blob("tame")), device=0, max_batch=16384)
    yield s
    s.close()


def see_positions(sp):
    from test_gpu_qsearch import generator_positions

    return np.concatenate([sp.positions_from_fens(SEE_FENS), generator_positions(sp)])


def test_device_see_equals_the_fixture_and_the_host_core(sp, st):
    """Every line of the fixture at its nine thresholds: spx_see == the compiled reference's bit == spx_pos_see."""
    from _see_rules import THRESHOLDS, read_fixture, word_to_uci

    entries, _ = read_fixture(FIXTURE)
    recs = sp.positions_from_fens([fen for fen, _ in entries])
    pos, words, thresholds, want = [], [], [], []
    for rec, (fen, masks) in zip(recs, entries):
        legal = sp.legal_moves(rec)[0]
        assert sorted(word_to_uci(w) for w in legal) == sorted(masks), fen
        for w in legal:
            mask = masks[word_to_uci(w)]
            for i, t in enumerate(THRESHOLDS):
                pos.append(rec)
                words.append(int(w))
                thresholds.append(t)
                want.append(bool((mask >> i) & 1))
    got = st.see(np.array(pos, dtype=sp.PACKED_DTYPE), np.array(words, dtype=np.uint16), np.array(thresholds, dtype=np.int32))
    want = np.array(want)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(sp.position_to_fen(pos[i]), word_to_uci(words[i]), thresholds[i]) for i in bad[:5]]
    host = np.array([sp.see(pos[i], words[i], thresholds[i]) for i in range(0, len(pos), 3)])
    assert np.array_equal(host, want[::3])
    print(f"{len(want)} triples, {int(want.sum())} true")
    assert len(want) > 360000 and 0.2 < want.mean() < 0.8


def test_device_see_equals_the_host_core_on_further_positions(sp, st):
    """>= 5 000 positions (goldens, hand-made, random playouts incl. DFRC) x every legal move x three thresholds."""
    pos = see_positions(sp)
    assert len(pos) >= 5000
    parents, words = [], []
    for i in range(len(pos)):
        legal = sp.legal_moves(pos[i])[0]
        parents += [i] * len(legal)
        words += [int(w) for w in legal]
    parents, words = np.array(parents), np.array(words, dtype=np.uint16)
    for threshold in (-81, 1, 300):
        got = st.see(pos[parents], words, threshold)
        want = np.array([sp.see(pos[p], w, threshold) for p, w in zip(parents, words)])
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (threshold, [(sp.position_to_fen(pos[parents[i]]), int(words[i])) for i in bad[:5]])
        print(f"threshold {threshold}: {len(want)} moves, {int(want.sum())} true")
        assert 0 < want.sum() < len(want)
    # an illegal move word is answered, not refused; no triples at all is fine too
    odd = st.see(pos[:4], np.array([0xFFFF, 0, 0x8000 | 4 | (7 << 6), 0x4000 | 12 | (21 << 6)], dtype=np.uint16), 0)
    assert odd.shape == (4,) and st.see(pos[:0], np.zeros(0, dtype=np.uint16), 0).shape == (0,)


def blocks(o, flags=False):
    return [(o["moves"][lo:lo + c].tobytes(), o["children"][lo:lo + c].tobytes(), bool(k)) +
            ((o["move_flags"][lo:lo + c].tobytes(),) if flags else ())
            for lo, c, k in zip(o["first"].tolist(), o["count"].tolist(), o["in_check"])]


def test_see_modes_and_flags_of_the_generator_match_the_python_predicates(sp, st):
    """Mixed modes 0-3, twice (position i in mode i % 4, then in mode (i % 4) ^ 1, so that every position is seen in modes 0 and 1
    or in modes 2 and 3): per position the children, move words, count, in_check, order, move_flags and pruned equal the host
    core's legal moves filtered and flagged by the Python predicates."""
    from _qsearch_rules import is_noisy
    from _see_rules import see

    pos = see_positions(sp)
    n = len(pos)
    cap = 64 * n + 256
    full = st.movegen(pos, capacity=cap)
    mails, stms = sp.positions_to_mailboxes(pos)
    expected = []
    for i in range(n):
        words, kids, chk = sp.legal_moves(pos[i])
        flags = [int(see(mails[i], int(stms[i]), w, -81)) | int(see(mails[i], int(stms[i]), w, 1)) << 1 |
                 int(is_noisy(pos[i], w)) << 2 for w in words]
        expected.append(([int(w) for w in words], [k.tobytes() for k in kids], bool(chk), flags))
    seen = {"mode 2 dropped": 0, "mode 3 dropped more than mode 2": 0, "in check unfiltered with see(-81) false": 0,
            "pruned en passant or promotion": 0, "every noisy move dropped": 0, "mode 0": 0, "mode 1": 0}
    pruned_by_mode = {}
    for round_, modes in enumerate(((np.arange(n) % 4).astype(np.uint8), ((np.arange(n) % 4) ^ 1).astype(np.uint8))):
        modes[:len(SEE_FENS)] = 3 - round_   # the hand-made positions in modes 3 and 2
        out = st.movegen(pos, capacity=cap, modes=modes, want_flags=True)
        assert int(out["count"].sum()) == len(out["children"]) == len(out["move_flags"])
        for i in range(n):
            words, kids, chk, flags = expected[i]
            mode = int(modes[i])
            cands = [k for k in range(len(words)) if mode == 0 or chk or flags[k] & 4]
            keep = cands if mode < 2 or chk else [k for k in cands if flags[k] & (1 if mode == 2 else 2)]
            want = sorted((words[k], kids[k], flags[k]) for k in keep)
            lo, cnt = int(out["first"][i]), int(out["count"][i])
            got = [(int(m), c.tobytes(), int(f)) for m, c, f in
                   zip(out["moves"][lo:lo + cnt], out["children"][lo:lo + cnt], out["move_flags"][lo:lo + cnt])]
            fen = sp.position_to_fen(pos[i])
            assert cnt == len(want) and sorted(got) == want, (fen, mode, got, want)
            assert int(out["pruned"][i]) == len(cands) - len(keep), (fen, mode)
            assert bool(out["in_check"][i]) == chk, fen
            assert np.all(out["parents"][lo:lo + cnt] == i)
            flo, fcnt = int(full["first"][i]), int(full["count"][i])
            wanted = {w for w, _, _ in want}
            assert [w for w, _, _ in got] == [int(m) for m in full["moves"][flo:flo + fcnt] if int(m) in wanted], fen
            pruned_by_mode[(i, mode)] = len(cands) - len(keep)
            dropped = [words[k] for k in cands if k not in keep]
            seen["mode 0"] += mode == 0
            seen["mode 1"] += mode == 1
            seen["mode 2 dropped"] += mode == 2 and len(dropped) > 0
            seen["in check unfiltered with see(-81) false"] += mode >= 2 and chk and any(not f & 1 for _, _, f in got)
            seen["pruned en passant or promotion"] += any(w >> 14 in (1, 3) for w in dropped)
            seen["every noisy move dropped"] += cnt == 0 and len(dropped) > 0
    seen["mode 3 dropped more than mode 2"] = sum(pruned_by_mode.get((i, 3), 0) > pruned_by_mode.get((i, 2), 1 << 30) for i in range(n))
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_flags_entry_point_writes_the_modes_entry_points_bytes(sp, st):
    """Modes 0 / 1 through spx_movegen_flags are spx_movegen_modes' bytes (and no modes at all spx_movegen's), pruned = 0;
    spx_movegen_modes with modes 2 / 3 gives the children of spx_movegen_flags; the device variants in a process of their own."""
    pos = see_positions(sp)[:1500]
    n = len(pos)
    cap = 64 * n + 256
    for modes in (None, np.zeros(n, dtype=np.uint8), (np.arange(n) % 2).astype(np.uint8)):
        a, b = st.movegen(pos, capacity=cap, modes=modes), st.movegen(pos, capacity=cap, modes=modes, want_flags=True)
        assert blocks(a) == blocks(b) and not b["pruned"].any()
    for i in (0, 1, 2, 700, n - 1):
        for mode in (0, 1):
            m = np.full(1, mode, dtype=np.uint8)
            a, b = st.movegen(pos[i:i + 1], modes=m), st.movegen(pos[i:i + 1], modes=m, want_flags=True)
            for key in ("children", "moves", "parents", "first", "count", "in_check"):
                assert a[key].tobytes() == b[key].tobytes(), (i, mode, key)
    modes = (2 + np.arange(n) % 2).astype(np.uint8)
    a, b = st.movegen(pos, capacity=cap, modes=modes), st.movegen(pos, capacity=cap, modes=modes, want_flags=True)
    assert blocks(a) == blocks(b) and b["pruned"].sum() > 0
    assert len(a["children"]) < len(st.movegen(pos, capacity=cap, modes=np.ones(n, dtype=np.uint8))["children"])


def test_device_variants_on_resident_buffers(sp):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "_see_device_worker.py")], cwd=root, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert "see device ok" in out.stdout


def test_capacity_overflow_is_reported_with_flags(sp, st):
    from stormphrax_amd import _lib

    pos = sp.random_positions(64, seed=3)
    with pytest.raises(_lib.SpxError) as err:
        st.movegen(pos, capacity=100, modes=np.zeros(64, dtype=np.uint8), want_flags=True)
    assert err.value.code == 5   # SPX_ERR_CAPACITY
