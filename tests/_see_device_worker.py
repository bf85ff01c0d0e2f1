"""Worker of tests/test_gpu_see.py::test_device_variants_on_resident_buffers (GPU box only): spx_see_device and
spx_movegen_flags_device on resident buffers against their host variants."""
import os
import sys

import numpy as np
import torch  # first: its HIP runtime must be the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormphrax_amd as sp  # noqa: E402
from stormphrax_amd import _lib  # noqa: E402


def blocks(o):
    return [(o["moves"][lo:lo + c].tobytes(), o["children"][lo:lo + c].tobytes(), o["move_flags"][lo:lo + c].tobytes(), bool(k), int(p))
            for lo, c, k, p in zip(o["first"].tolist(), o["count"].tolist(), o["in_check"], o["pruned"].tolist())]


def main():
    pos = np.concatenate([sp.random_positions(1200, seed=41, min_ply=0, max_ply=200, dfrc_every=2),
                          sp.random_positions(300, seed=42, min_ply=0, max_ply=14, dfrc_every=1)])
    n = len(pos)
    cap = 64 * n + 256
    modes = (np.arange(n) % 4).astype(np.uint8)
    lib = _lib.load()
    with sp.NnueState(sp.Network(sp.synthetic_net_bytes("tame")), device=0, max_batch=4096) as st:
        host = st.movegen(pos, capacity=cap, modes=modes, want_flags=True)
        assert int(host["pruned"].sum()) > 0
        d_pos = torch.from_numpy(pos.view(np.uint8).reshape(-1, 32).copy()).cuda()
        d_modes = torch.from_numpy(modes).cuda()
        d_children = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
        d_moves = torch.zeros(cap, dtype=torch.int16, device="cuda")
        d_parents = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_flags = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_first = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_count = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_check = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_pruned = torch.zeros(n, dtype=torch.int16, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.spx_movegen_flags_device(st._h, d_pos.data_ptr(), d_modes.data_ptr(), n, None, d_children.data_ptr(),
                                                d_moves.data_ptr(), d_parents.data_ptr(), d_first.data_ptr(), d_count.data_ptr(),
                                                d_check.data_ptr(), d_flags.data_ptr(), d_pruned.data_ptr(), cap, d_total.data_ptr(),
                                                stream))
        torch.cuda.synchronize()
        total = int(d_total.item())
        assert total == len(host["children"]), (total, len(host["children"]))
        got = {"children": d_children.cpu().numpy()[:total].copy().view(sp.PACKED_DTYPE).reshape(-1),
               "moves": d_moves.cpu().numpy()[:total].view(np.uint16), "move_flags": d_flags.cpu().numpy()[:total],
               "first": d_first.cpu().numpy().view(np.uint32), "count": d_count.cpu().numpy().view(np.uint32),
               "in_check": d_check.cpu().numpy(), "pruned": d_pruned.cpu().numpy().view(np.uint16)}
        assert blocks(got) == blocks(host)

        # spx_see_device: every child's move at its parent, three thresholds
        parents = pos[host["parents"]]
        words = host["moves"]
        for threshold in (-81, 1, 434):
            want = st.see(parents, words, threshold)
            d_par = torch.from_numpy(parents.view(np.uint8).reshape(-1, 32).copy()).cuda()
            d_words = torch.from_numpy(words.view(np.int16).copy()).cuda()
            d_thr = torch.full((len(words),), threshold, dtype=torch.int32, device="cuda")
            d_ok = torch.full((len(words),), 7, dtype=torch.uint8, device="cuda")
            _lib.check(lib.spx_see_device(st._h, d_par.data_ptr(), d_words.data_ptr(), d_thr.data_ptr(), len(words), d_ok.data_ptr(),
                                          stream))
            torch.cuda.synchronize()
            assert np.array_equal(d_ok.cpu().numpy().astype(bool), want) and 0 < want.sum() < len(want)
    print("see device ok")


if __name__ == "__main__":
    main()
