"""Plain-Python restatement of the PRUNED quiescence node (SPX_SELFPLAY_QUIESCE_PRUNING; the rules are with SearchStepParams in
stormphrax_amd/csrc/spx_kernels.h; the reference is qsearch, src/search.cpp:1451-1640). TEST INFRASTRUCTURE: QSearcher of
tests/_qsearch_rules.py with the node below, literally - the candidates are filtered and flagged HERE, from is_noisy and the
Python static exchange evaluation of tests/_see_rules.py; nothing is shared with the device's generator modes, its move flags or
the step kernel's frames.

  fut = stand + 142 (qsearchFpMargin);  loss = a score below -K_SCORE_WIN
  quiesce(c, stand, a, b, ply, q):
    q == 0 -> stand;  stand >= b -> stand
    expand c: in check every legal move; else the noisy moves that pass see(m, 1) if fut <= max(a, stand) ("mode 3"), else
      those that pass see(m, -81) ("mode 2"); pruned = the noisy moves dropped
    in check, no candidate -> -(MATE - ply);  in check: best = -INF;  else best = stand, a = max(a, stand)
    not in check, mode 3, pruned > 0: best = max(best, fut)
    searched = 0;  candidates by (value descending, move word ascending), for each m:
      if best is not a loss:
        not in check and fut <= a and not see(m, 1): best = max(best, fut); continue
        searched >= 2: stop
        in check and m is not noisy: continue
        not see(m, -81): continue
      searched += 1;  x = -quiesce(child, -value(child), -b, -a, ply + 1, q - 1);  fail-soft, stop at a >= b
    return best

`branches` switches each pruning rule on or off (all off = QSearcher, node for node); `taken` counts how often each fired."""
import numpy as np

from _datagen_rules import K_SCORE_WIN, clamp_static
from _qsearch_rules import QSearcher, is_noisy, verify_qsearch_file
from _search_rules import INF, MATE
from _see_rules import see

FP_MARGIN = 142        # qsearchFpMargin, tunable.h:377
SEE_THRESHOLD = -81    # qsearchSeeThreshold, tunable.h:378
ALL_BRANCHES = ("generator see", "generator futility", "futility after alpha rose", "cap", "quiet evasion", "losing evasion")


class PrunedQSearcher(QSearcher):
    def __init__(self, sp, st, budget, quiesce_plies, branches=ALL_BRANCHES):
        super().__init__(sp, st, budget, quiesce_plies)
        self.branches = set(branches)
        self.taken = {name: 0 for name in ALL_BRANCHES + ("lifted by dropped moves", "cap in check", "cap out of check",
                                                          "first evasion searched as a loss")}
        self.flag_cache = {}

    def flags_of(self, rec):
        """-> (words, kids, in_check, [see(-81) | see(1) << 1 | noisy << 2 per legal move])."""
        key = rec.tobytes()
        hit = self.flag_cache.get(key)
        if hit is None:
            words, kids, in_check = self.sp.legal_moves(rec)
            mail, stm = self.sp.positions_to_mailboxes(np.array([rec]))
            flags = [int(see(mail[0], int(stm[0]), w, SEE_THRESHOLD)) | int(see(mail[0], int(stm[0]), w, 1)) << 1 |
                     int(is_noisy(rec, w)) << 2 for w in words]
            hit = (words, kids, bool(in_check), flags)
            self.flag_cache[key] = hit
        return hit

    def expand_pruned(self, rec, futile):
        """One quiescence node: -> (kids, values, in_check, order, flags, pruned)."""
        key = (rec.tobytes(), futile)
        hit = self.qcache.get(key)
        if hit is None:
            words, kids, in_check, flags = self.flags_of(rec)
            cands = [i for i in range(len(words)) if in_check or flags[i] & 4]
            keep = cands
            if not in_check and futile and "generator futility" in self.branches:
                keep = [i for i in cands if flags[i] & 2]
            elif not in_check and "generator see" in self.branches:
                keep = [i for i in cands if flags[i] & 1]
            values = {}
            if keep:
                raw = self.st.evaluate_once(kids[keep])
                values = {i: clamp_static(-int(v)) for i, v in zip(keep, raw)}
                if len(self.leaves) < 200000:
                    self.leaves.extend((kids[i].tobytes(), int(v)) for i, v in list(zip(keep, raw))[::7])
            order = sorted(keep, key=lambda i: (-values[i], int(words[i])))
            hit = (kids, values, in_check, order, flags, len(cands) - len(keep), len(words))
            self.qcache[key] = hit
        self.nodes += 1
        self.expanded += 1
        self.quiesce_nodes += 1
        self.candidates += len(hit[3])
        self.legal += hit[6]
        return hit[:6]

    def quiesce(self, rec, stand, a, b, ply, q):
        if q == 0:
            return stand
        if stand >= b and self.stand_pat_cuts_unexpanded(rec):
            return stand
        self.deepest_quiesce = max(self.deepest_quiesce, self.q - q + 1)
        fut = stand + FP_MARGIN
        futile = fut <= max(a, stand)
        kids, values, in_check, order, flags, pruned = self.expand_pruned(rec, futile)
        if in_check and not order:
            return -(MATE - ply)
        if in_check:
            best = -INF
        else:
            best = stand
            a = max(a, stand)
            if futile and pruned > 0:
                best = max(best, fut)
                self.taken["lifted by dropped moves"] += 1
                self.taken["generator futility"] += 1
            elif pruned > 0:
                self.taken["generator see"] += 1
        searched = 0
        for i in order:
            if best >= -K_SCORE_WIN:
                if "futility after alpha rose" in self.branches and not in_check and fut <= a and not flags[i] & 2:
                    best = max(best, fut)
                    self.taken["futility after alpha rose"] += 1
                    continue
                if "cap" in self.branches and searched >= 2:
                    self.taken["cap"] += 1
                    self.taken["cap in check" if in_check else "cap out of check"] += 1
                    break
                if "quiet evasion" in self.branches and in_check and not flags[i] & 4:
                    self.taken["quiet evasion"] += 1
                    continue
                if "losing evasion" in self.branches and not flags[i] & 1:   # (out of check the generator has dropped these)
                    self.taken["losing evasion"] += 1
                    continue
            elif in_check and searched == 0:
                self.taken["first evasion searched as a loss"] += 1
            searched += 1
            x = -self.quiesce(kids[i], -values[i], -b, -a, ply + 1, q - 1)
            if x > best:
                best = x
            if x > a:
                a = x
            if a >= b:
                break
        return best


def verify_qprune_file(sp, st, oracle, blob, max_plies, budget, quiesce_plies, tally=None, plain=None):
    """verify_qsearch_file with the pruned searcher; `plain`, if given, receives per ply whether the UNPRUNED quiescence search
    (QSearcher, same budget and plies) would have played another move.
    verify_qsearch_file builds its searcher by the name _qsearch_rules.QSearcher and has no parameter for another class; that
    module is shared with the existing quiescence tests and is left as it is, so the name is pointed at the pruned searcher for the
    duration of the call and restored afterwards (one process, no threads: nothing else can see the swap)."""
    import _qsearch_rules

    unpruned = QSearcher(sp, st, budget, quiesce_plies) if plain is not None else None
    made = []

    class Recording(PrunedQSearcher):
        def __init__(self, *args):
            super().__init__(*args)
            made.append(self)

        def root(self, rec):
            out = super().root(rec)
            if unpruned is not None:
                plain.append(unpruned.root(rec)[0] != out[0])
            return out

    original = _qsearch_rules.QSearcher
    _qsearch_rules.QSearcher = Recording
    try:
        checked, searcher, deepest = verify_qsearch_file(sp, st, oracle, blob, max_plies, budget, quiesce_plies, tally)
    finally:
        _qsearch_rules.QSearcher = original
    assert searcher is made[0]
    return checked, searcher, deepest, unpruned
