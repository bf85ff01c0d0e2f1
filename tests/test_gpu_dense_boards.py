"""Dense boards through the column-sliced pipeline: 32 pieces, promoted queens, many pawn pairs.

spx_ftx_extract_kernel turns a position's (attacker, victim) pairs and pawn pairs into rows 64 items per round; the boards of
game play need one round, these need several. Their lists run up to the caps (32 piece-square rows, 256 threat / pawn-pair rows),
and the sums must still equal the one-kernel path (SPX_CTX_ONE_KERNEL_FT) and the CPU oracle bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXED = [
    "qqqqkqqq/pppppppp/8/8/8/8/PPPPPPPP/QQQQKQQQ w - - 0 1",
    "1q1q1q1k/p1p1p1p1/1P1P1P1P/Q1Q1Q1Q1/1q1q1q1q/p1p1p1p1/1P1P1P1P/K1Q1Q1Q1 w - - 0 1",
    "r1bqkb1r/pppppppp/2Q2Q2/8/8/2q2q2/PPPPPPPP/R1BQKB1R b - - 0 1",
    "k7/pppp4/PPPP4/4pppp/4PPPP/pppp4/PPPP4/7K w - - 0 1",
]


def _dense_fens(n, seed):
    """Random boards with both kings and 30 more pieces, queens the most common: many attackers with many targets each."""
    rng = np.random.default_rng(seed)
    kinds = np.array(list("QqRrBbNnPp"))
    weights = np.array([6, 6, 2, 2, 2, 2, 2, 2, 4, 4], dtype=float)
    fens = []
    for _ in range(n):
        board = [""] * 64
        squares = rng.permutation(64)
        board[squares[0]], board[squares[1]] = "K", "k"
        placed = 0
        for sq in squares[2:]:
            if placed == 30:
                break
            piece = rng.choice(kinds, p=weights / weights.sum())
            if piece in "Pp" and sq // 8 in (0, 7):
                piece = "Q" if piece == "P" else "q"
            board[sq] = piece
            placed += 1
        ranks = []
        for r in range(7, -1, -1):
            row, empty = "", 0
            for f in range(8):
                p = board[8 * r + f]
                if p:
                    row += (str(empty) if empty else "") + p
                    empty = 0
                else:
                    empty += 1
            ranks.append(row + (str(empty) if empty else ""))
        fens.append("/".join(ranks) + (" w" if rng.integers(2) else " b") + " - - 0 1")
    return fens


@pytest.mark.parametrize("preset", ["tame", "realistic"])
def test_dense_boards_through_the_sliced_pipeline(sp, oracle, net_blob, preset):
    fens = FIXED + _dense_fens(4096 - len(FIXED), seed=7)
    pos = sp.positions_from_fens(fens)
    blob = net_blob(preset)
    with sp.NnueState(sp.Network(blob), device=0, max_batch=4096, sliced_ft=False) as plain, \
            sp.NnueState(sp.Network(blob), device=0, max_batch=4096,
                         options={"ftx_min": 1024, "tiny_batch_max": 0, "mlp_share_max": 0}) as sliced:
        assert sliced.takes_sliced_pipeline(len(pos)) and not plain.takes_sliced_pipeline(len(pos))
        got = sliced.evaluate_once(pos)
        lists = sliced.ftx_lists(len(pos))
        want = plain.evaluate_once(pos)
    thr = np.array([len(t) for _, t, _ in lists])
    psq = np.array([len(p) for p, _, _ in lists])
    assert (psq == 32).mean() > 0.99
    assert (thr >= 64).mean() > 0.9 and thr.max() >= 96  # more than one round of 64 items per position
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} differ from the one-kernel path, first: {fens[bad[0]]}"
    oracle.use(blob, preset)
    mail, stm = sp.positions_to_mailboxes(pos)
    bad = np.nonzero(got != oracle.eval_mailboxes(mail, stm))[0]
    assert bad.size == 0, f"{bad.size} differ from the CPU oracle, first: {fens[bad[0]]}"
