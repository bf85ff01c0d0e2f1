"""Plain-Python restatement of the static exchange evaluation (spx_pos_see / spx_see; the reference's see::see, src/see.cpp:44-132)
on a record's MAILBOX (stormphrax_amd.positions_to_mailboxes: 64 piece ids, type << 1 | colour with white = 1, 12 = empty).
TEST INFRASTRUCTURE in the style of _qsearch_rules.is_noisy: ray walks square by square, nothing shared with the bitboard code of
the host chess core or of the device. tests/golden/see.txt.gz holds the compiled reference's own answers.

  gain(move)      castling 0; en passant a pawn; else value(piece on the target) [+ value(promoted) - value(pawn)]
  see(move, t)    score = gain - t;  score < 0 -> no;  score -= value(moving piece, or the promoted one);  score >= 0 -> yes
                  occupancy = the position's with `from` and `to` toggled (an en-passant victim stays on the board)
                  attackers of `to`, both colours, restricted by the pins of the position BEFORE the move: a pinned piece (the
                    single own piece between its king and an enemy slider, rays cut by enemy pieces only) counts only if it stands
                    on the line through its king and `to`
                  sides alternate, the opponent first: no attacker -> stop; the least valuable attacker (pawn, knight, bishop,
                    rook, queen, king; lowest square first) leaves the occupancy; after a pawn, bishop or queen the diagonal
                    sliders now seeing `to` join, after a rook or queen the orthogonal ones (x-rays, NOT pin-restricted);
                    score = -score - 1 - value(that piece); once score >= 0 the side to act next has lost the exchange - unless
                    the piece that just captured was a king and the side to act still has an attacker: then the king's side has
                  yes iff the side that lost is not the mover's"""

VALUE = (97, 434, 464, 646, 1289, 0)  # tunable.h:155-159
THRESHOLDS = (-1289, -646, -81, -1, 0, 1, 97, 434, 1000)  # the fixture's threshold list, bit i of a mask = T[i]
EMPTY = 12
DIAG = ((1, 1), (1, -1), (-1, 1), (-1, -1))
ORTH = ((1, 0), (-1, 0), (0, 1), (0, -1))
KNIGHT = ((1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2))


def _walk(sq, step):
    f, r = sq & 7, sq >> 3
    while True:
        f, r = f + step[0], r + step[1]
        if not (0 <= f < 8 and 0 <= r < 8):
            return
        yield r * 8 + f


def _same_line(a, b, c):
    """c stands on the line (file, rank or diagonal) through the two distinct aligned squares a and b."""
    if a == b:
        return False
    for key in (lambda s: s & 7, lambda s: s >> 3, lambda s: (s & 7) - (s >> 3), lambda s: (s & 7) + (s >> 3)):
        if key(a) == key(b):
            return key(c) == key(a)
    return False


def pinned_squares(mail, colour):
    king = next(sq for sq in range(64) if mail[sq] == (10 | colour))
    pinned = set()
    for steps, sliders in ((DIAG, (2, 4)), (ORTH, (3, 4))):
        for step in steps:
            own = []
            for sq in _walk(king, step):
                piece = int(mail[sq])
                if piece == EMPTY:
                    continue
                if (piece & 1) == colour:
                    own.append(sq)   # own pieces do not cut the ray
                    continue
                if (piece >> 1) in sliders and len(own) == 1:
                    pinned.add(own[0])
                break                # the first enemy piece does
    return pinned, king


def _slider_attackers(mail, to, occ, steps, sliders):
    found = set()
    for step in steps:
        for sq in _walk(to, step):
            if sq in occ:
                if (int(mail[sq]) >> 1) in sliders:
                    found.add(sq)
                break
    return found


def see(mail, stm, word, threshold):
    """mail: 64 piece ids of the position, stm: 1 = white to move, word: viriformat move word (assumed legal)."""
    word = int(word)
    frm, to, kind = word & 63, (word >> 6) & 63, word >> 14  # 0 normal, 1 en passant, 2 castling, 3 promotion
    promo = ((word >> 12) & 3) + 1
    if kind == 2:
        score = 0
    elif kind == 1:
        score = VALUE[0]
    else:
        score = 0 if mail[to] == EMPTY else VALUE[int(mail[to]) >> 1]
        if kind == 3:
            score += VALUE[promo] - VALUE[0]
    score -= threshold
    if score < 0:
        return False
    score -= VALUE[promo] if kind == 3 else VALUE[int(mail[frm]) >> 1]
    if score >= 0:
        return True

    occ = {sq for sq in range(64) if mail[sq] != EMPTY}
    occ ^= {frm}
    occ ^= {to}
    attackers = _slider_attackers(mail, to, occ, DIAG, (2, 4)) | _slider_attackers(mail, to, occ, ORTH, (3, 4))
    f, r = to & 7, to >> 3
    for df, dr in KNIGHT:
        if 0 <= f + df < 8 and 0 <= r + dr < 8 and int(mail[(r + dr) * 8 + f + df]) >> 1 == 1:
            attackers.add((r + dr) * 8 + f + df)
    for df in (-1, 0, 1):
        for dr in (-1, 0, 1):
            if (df or dr) and 0 <= f + df < 8 and 0 <= r + dr < 8 and int(mail[(r + dr) * 8 + f + df]) >> 1 == 5:
                attackers.add((r + dr) * 8 + f + df)
    for df in (-1, 1):
        if 0 <= f + df < 8:
            if r >= 1 and mail[(r - 1) * 8 + f + df] == 1:   # a white pawn one rank below attacks upwards
                attackers.add((r - 1) * 8 + f + df)
            if r <= 6 and mail[(r + 1) * 8 + f + df] == 0:   # a black pawn one rank above
                attackers.add((r + 1) * 8 + f + df)
    for colour in (0, 1):
        pinned, king = pinned_squares(mail, colour)
        attackers -= {sq for sq in pinned if not _same_line(king, to, sq)}

    side = stm ^ 1
    while True:
        ours = [sq for sq in attackers if (int(mail[sq]) & 1) == side]
        if not ours:
            break
        sq = min(ours, key=lambda s: (int(mail[s]) >> 1, s))
        piece = int(mail[sq]) >> 1
        occ.discard(sq)
        if piece in (0, 2, 4):
            attackers |= _slider_attackers(mail, to, occ, DIAG, (2, 4))
        if piece in (3, 4):
            attackers |= _slider_attackers(mail, to, occ, ORTH, (3, 4))
        attackers &= occ
        score = -score - 1 - VALUE[piece]
        side ^= 1
        if score >= 0:
            if piece == 5 and any((int(mail[s]) & 1) == side for s in attackers):
                side ^= 1
            break
    return side != stm


def word_to_uci(word):
    """The fixture's move text: from, to (castling: the own rook's square), promotion letter."""
    word = int(word)
    frm, to = word & 63, (word >> 6) & 63
    text = "abcdefgh"[frm & 7] + str((frm >> 3) + 1) + "abcdefgh"[to & 7] + str((to >> 3) + 1)
    return text + ("nbrq"[(word >> 12) & 3] if word >> 14 == 3 else "")


def read_fixture(path):
    """-> [(fen, {uci: mask})] of tests/golden/see.txt.gz, and the index of the first hand-made position."""
    import gzip

    out, hand = [], None
    with gzip.open(path, "rt") as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith("#"):
                if "section hand-made" in line:
                    hand = len(out)
                continue
            if line.startswith("F "):
                out.append((line[2:], {}))
            elif line:
                uci, mask = line.split()
                out[-1][1][uci] = int(mask)
    return out, hand
