"""Static exchange evaluation on the CPU: the plain-Python restatement (tests/_see_rules.py) and the host chess core
(spx_pos_see) against tests/golden/see.txt.gz - the compiled reference's own see::see for every legal move of 1 564 positions at
nine thresholds - and the hand-made positions of the fixture once more with the expected bit and its reason written here, so that
a wrong fixture would show."""
import os

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "see.txt.gz")


@pytest.fixture(scope="module")
def fixture_lines(sp):
    """-> [(record, mailbox, stm, {uci: (move word, mask)})], index of the first hand-made position."""
    from _see_rules import read_fixture, word_to_uci

    entries, hand = read_fixture(FIXTURE)
    assert len(entries) >= 1500 and hand is not None and len(entries) - hand == 12
    recs = sp.positions_from_fens([fen for fen, _ in entries])
    mails, stms = sp.positions_to_mailboxes(recs)
    out = []
    for rec, mail, stm, (fen, masks) in zip(recs, mails, stms, entries):
        words = sp.legal_moves(rec)[0]
        by_uci = {word_to_uci(w): int(w) for w in words}
        assert sorted(by_uci) == sorted(masks), fen   # the host core's legal moves are the reference's
        out.append((rec, mail, int(stm), {uci: (by_uci[uci], mask) for uci, mask in masks.items()}))
    return out, hand


def test_the_restatement_equals_every_line_of_the_fixture(fixture_lines):
    from _see_rules import THRESHOLDS, see

    lines, _ = fixture_lines
    checked = 0
    for _, mail, stm, moves in lines:
        for uci, (word, mask) in moves.items():
            got = sum(1 << i for i, t in enumerate(THRESHOLDS) if see(mail, stm, word, t))
            assert got == mask, (uci, got, mask)
            checked += 1
    print(f"{checked} moves x {len(THRESHOLDS)} thresholds")
    assert checked > 40000


def test_the_host_core_equals_every_line_of_the_fixture(sp, fixture_lines):
    from _see_rules import THRESHOLDS

    lines, _ = fixture_lines
    both = {0: 0, 1: 0}
    for rec, _, _, moves in lines:
        for uci, (word, mask) in moves.items():
            for i, t in enumerate(THRESHOLDS):
                got = sp.see(rec, word, t)
                assert got == bool((mask >> i) & 1), (sp.position_to_fen(rec), uci, t)
                both[int(got)] += 1
    assert min(both.values()) > 50000, both


# (fen, move, threshold, expected, why) - each also a line of the fixture's hand-made section
HAND_MADE = [
    ("4k3/2p5/8/3pP3/8/8/8/4K3 w - d6 0 1", "e5d6", 0, True, "en passant gains a pawn (97), c7 takes it back: 0"),
    ("4k3/2p5/8/3pP3/8/8/8/4K3 w - d6 0 1", "e5d6", 1, False, "... which is not 1"),
    ("4k3/P7/8/8/8/8/8/4K3 w - - 0 1", "a7a8q", 1000, True, "a quiet promotion gains queen - pawn = 1192, nobody recaptures"),
    ("4k3/P7/8/8/8/8/8/4K3 w - - 0 1", "a7a8n", 434, False, "knight - pawn = 337 < 434"),
    ("4k3/P7/8/8/8/8/8/4K3 w - - 0 1", "a7a8r", 434, True, "rook - pawn = 549 >= 434"),
    ("1n1rk3/P7/8/8/8/8/8/4K3 w - - 0 1", "a7b8q", 97, True, "capturing promotion: knight + 1192, then the rook takes the QUEEN (1289): 337"),
    ("1n1rk3/P7/8/8/8/8/8/4K3 w - - 0 1", "a7b8q", 434, False, "... 337 < 434: the exchange continues with the promoted piece"),
    ("4k3/8/8/8/8/8/8/R3K2R w KQ - 0 1", "e1h1", 0, True, "castling gains 0 (its target square holds the own rook)"),
    ("4k3/8/8/8/8/8/8/R3K2R w KQ - 0 1", "e1a1", 1, False, "castling gains 0"),
    ("4k3/8/4p3/3p4/8/8/8/3RR1K1 w - - 0 1", "d1d5", 97, True, "the defender e6 is pinned to e8 by Re1 and d5 is off that file: Rxd5 wins the pawn"),
    ("4k3/3p4/8/8/B7/2Q5/8/6K1 w - - 0 1", "c3c6", -646, False, "d7 is pinned by Ba4 but c6 lies on the line a4-e8: it may take the queen (-1289 + 97)"),
    ("4k3/3p4/8/8/B7/2Q5/8/6K1 w - - 0 1", "c3c6", -1289, True, "... and -1289 is the worst that can happen"),
    ("4k3/2b5/3p4/4p3/3P4/2B5/8/4K3 w - - 0 1", "d4e5", 1, False, "x-ray through a pawn: after d6xe5, Bxe5 the bishop c7 behind d6 recaptures: 0"),
    ("4k3/2b5/3p4/4p3/3P4/2B5/8/4K3 w - - 0 1", "d4e5", 0, True, "... and 0 >= 0"),
    ("4k2q/6b1/8/4p3/3P4/5N2/8/4K3 w - - 0 1", "d4e5", 97, False, "x-ray through a bishop: the queen h8 behind g7 takes the knight back: 97 - 97 + 464 - 434 = 30"),
    ("4k2q/6b1/8/4p3/3P4/5N2/8/4K3 w - - 0 1", "d4e5", 1, True, "... 30 >= 1"),
    ("3rk3/3r4/8/3p4/8/8/3R4/3RK3 w - - 0 1", "d2d5", -81, False, "x-ray through a rook: the second black rook is counted, white ends a rook for a pawn down"),
    ("3rk3/3r4/8/3p4/8/8/3R4/3RK3 w - - 0 1", "d2d5", -646, True, "... 97 - 646 = -549 >= -646"),
    ("3rk3/3q4/8/3p4/8/8/3R4/3QK3 w - - 0 1", "d2d5", -81, False, "x-ray through a queen on a file: the rook d8 behind the queen d7 recaptures last"),
    ("4k3/8/8/8/8/1n6/3r4/3RK3 w - - 0 1", "d1d2", 434, True, "RxR, NxR, and the king, the last attacker, takes the knight: nobody defends it"),
    ("4k3/8/8/b7/8/1n6/3r4/3RK3 w - - 0 1", "d1d2", 1, False, "the same with Ba5 behind: the king may not take a defended knight, rook for rook = 0"),
    ("4k3/8/8/b7/8/1n6/3r4/3RK3 w - - 0 1", "d1d2", 0, True, "... and 0 >= 0"),
]


def test_hand_made_positions_one_per_special_rule(sp, fixture_lines):
    from _see_rules import THRESHOLDS, read_fixture, see, word_to_uci

    entries, hand = read_fixture(FIXTURE)
    in_fixture = {fen: masks for fen, masks in entries[hand:]}
    for fen, uci, threshold, expected, why in HAND_MADE:
        rec = sp.positions_from_fens([fen])[0]
        word = next(int(w) for w in sp.legal_moves(rec)[0] if word_to_uci(w) == uci)
        mail, stm = sp.positions_to_mailboxes(np.array([rec]))
        assert sp.see(rec, word, threshold) == expected, (fen, uci, threshold, why)
        assert see(mail[0], int(stm[0]), word, threshold) == expected, (fen, uci, threshold, why)
        assert bool((in_fixture[fen][uci] >> THRESHOLDS.index(threshold)) & 1) == expected, (fen, uci, threshold, why)


def test_an_illegal_move_word_is_answered_not_refused(sp):
    """The move is assumed legal; anything else gives an unspecified bool (here: an empty from-square, a capture of the own king)."""
    rec = sp.positions_from_fens(["4k3/8/8/8/8/8/8/4K3 w - - 0 1"])[0]
    for word in (20 | (28 << 6), 4 | (4 << 6), 0xFFFF, 0x8000 | 4 | (7 << 6), 0x4000 | 12 | (21 << 6)):
        assert sp.see(rec, word, 0) in (True, False)


def test_argument_errors_of_the_host_entry_point(sp):
    """A NULL argument is SPX_ERR_INVALID_ARG (1), a record that does not unpack SPX_ERR_BAD_POSITION."""
    import ctypes

    from stormphrax_amd import _lib

    lib = _lib.load()
    rec = sp.positions_from_fens(["4k3/8/8/8/8/8/8/4K3 w - - 0 1"])
    ok = ctypes.c_int()
    assert lib.spx_pos_see(None, 0, 0, ctypes.byref(ok)) == 1
    assert lib.spx_pos_see(rec.ctypes.data, 0, 0, None) == 1
    bad = rec.copy()
    bad["occupancy"] = 0   # no kings
    assert lib.spx_pos_see(bad.ctypes.data, 0, 0, ctypes.byref(ok)) not in (0, 1)
