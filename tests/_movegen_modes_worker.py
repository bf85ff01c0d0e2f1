"""Worker of tests/test_gpu_qsearch.py::test_mode_zero_and_no_modes_are_the_plain_generator_and_the_device_variant_agrees (GPU
box only): spx_movegen_modes_device on resident buffers against the host variant."""
import os
import sys

import numpy as np
import torch  # first: its HIP runtime must be the one the process initialises

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormphrax_amd as sp  # noqa: E402
from stormphrax_amd import _lib  # noqa: E402


def blocks(o):
    return [(o["moves"][lo:lo + c].tobytes(), o["children"][lo:lo + c].tobytes(), bool(k))
            for lo, c, k in zip(o["first"].tolist(), o["count"].tolist(), o["in_check"])]


def main():
    pos = np.concatenate([sp.random_positions(1200, seed=41, min_ply=0, max_ply=200, dfrc_every=2),
                          sp.random_positions(300, seed=42, min_ply=0, max_ply=14, dfrc_every=1)])
    n = len(pos)
    cap = 64 * n + 256
    modes = (np.arange(n) % 2).astype(np.uint8)
    lib = _lib.load()
    with sp.NnueState(sp.Network(sp.synthetic_net_bytes("tame")), device=0, max_batch=4096) as st:
        plain = st.movegen(pos, capacity=cap)
        host = st.movegen(pos, capacity=cap, modes=modes)
        assert len(host["children"]) < len(plain["children"])
        d_pos = torch.from_numpy(pos.view(np.uint8).reshape(-1, 32).copy()).cuda()
        d_modes = torch.from_numpy(modes).cuda()
        d_children = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
        d_moves = torch.zeros(cap, dtype=torch.int16, device="cuda")
        d_parents = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_first = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_count = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_check = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for d_m, want in ((d_modes.data_ptr(), host), (None, plain)):
            _lib.check(lib.spx_movegen_modes_device(st._h, d_pos.data_ptr(), d_m, n, None, d_children.data_ptr(),
                                                    d_moves.data_ptr(), d_parents.data_ptr(), d_first.data_ptr(), d_count.data_ptr(),
                                                    d_check.data_ptr(), cap, d_total.data_ptr(), stream))
            torch.cuda.synchronize()
            total = int(d_total.item())
            assert total == len(want["children"]), (total, len(want["children"]))
            got = {"children": d_children.cpu().numpy()[:total].copy().view(sp.PACKED_DTYPE).reshape(-1),
                   "moves": d_moves.cpu().numpy()[:total].view(np.uint16), "first": d_first.cpu().numpy().view(np.uint32),
                   "count": d_count.cpu().numpy().view(np.uint32), "in_check": d_check.cpu().numpy()}
            assert blocks(got) == blocks(want)
    print("modes device ok")


if __name__ == "__main__":
    main()
