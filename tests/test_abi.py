"""The C-ABI library loads and exports every symbol include/spx_nnue.h (the drop-in boundary) declares - and nothing else -; its
dev build (libspx_nnue_dev.so: the same objects plus the test / measurement entry points of include/spx_nnue_dev.h) exports both
headers' symbols (no compute calls without a GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="spx_nnue.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(spx_[a-z0-9_]+)\s*\(", text)))


def exported_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.split()[-2] in "TWBDR")


def test_header_and_library_agree(sp):
    from stormphrax_amd import _lib

    lib = _lib.load()
    names, dev = declared_symbols(), declared_symbols("spx_nnue_dev.h")
    assert len(names) >= 18 and len(dev) >= 12 and not set(names) & set(dev)
    # the boundary header carries no test scaffolding
    assert not [n for n in names if "debug" in n or "probe" in n or "synth" in n or "random" in n or "perft" in n]
    for name in names + dev:
        assert hasattr(lib, name), f"{name} is declared in include/ but not exported"
    assert sorted(_lib.SYMBOLS) == sorted(names + dev), "ctypes prototypes drifted from the headers"
    assert ctypes.sizeof(_lib.PackedPos) == 32 and sp.PACKED_DTYPE.itemsize == 32


def test_product_library_exports_the_boundary_and_nothing_else():
    """libspx_nnue.so - what an engine links - exports exactly the functions of include/spx_nnue.h: no
    spx_debug_*, no probe kernels' launchers, no synthetic nets, no C++ internals. The dev build exports the dev header on top."""
    from stormphrax_amd import _lib

    names, dev = declared_symbols(), declared_symbols("spx_nnue_dev.h")
    product = exported_symbols(_lib.PRODUCT_PATH)
    assert product == names, sorted(set(product) ^ set(names))
    assert not [n for n in product if "debug" in n or "probe" in n]
    exported_dev = set(exported_symbols(_lib.LIB_PATH))
    assert set(names + dev) <= exported_dev
    handle = ctypes.CDLL(_lib.PRODUCT_PATH)  # loads on its own (no unresolved reference into the dev build)
    assert all(hasattr(handle, n) for n in names) and not hasattr(handle, "spx_debug_copy_ft")


def test_no_cpu_fallback_without_device(sp, net_blob):
    """On a box without a GPU the context must refuse to exist (SPX_ERR_NO_DEVICE): there is no CPU evaluation path."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from stormphrax_amd import _lib

    net = sp.Network(net_blob("tame"))
    with pytest.raises(_lib.SpxError) as err:
        sp.NnueState(net, device=0, max_batch=16)
    assert err.value.code == 4 and "no CPU fallback" in str(err.value)
    # the multi-device group refuses the same way, with every visible device (none) as well as a named one
    assert sp.device_count() == 0
    for devices in (None, [0], [0, 1]):
        with pytest.raises(_lib.SpxError) as err:
            sp.DeviceGroup(net, devices=devices, max_batch_per_device=16)
        assert err.value.code == 4


def test_product_never_references_the_oracle():
    """The shipped sources must not include, link or load anything under oracle/."""
    for sub in ("stormphrax_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for name in files:
                if name.endswith((".cpp", ".h", ".hip", ".py", "Makefile")):
                    text = open(os.path.join(dirpath, name), errors="replace").read()
                    assert "libspx_oracle" not in text and "spxo_" not in text and "oracle/" not in text.replace(
                        "the CPU oracle lives in oracle/", ""), os.path.join(dirpath, name)


def test_cpp_mirror_header_compiles_standalone():
    """include/spx_nnue.hpp (the C++ mirror of eval::NnueState) is self-contained: it compiles with a plain host
    compiler, without HIP headers, against the C ABI header alone."""
    import subprocess

    src = '#include "spx_nnue.hpp"\nint main() { return sizeof(spx_nnue::NnueState) > 0 ? 0 : 1; }\n'
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                          os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_bench_refuses_to_run_without_a_gpu():
    """The evaluator has no CPU path: on a box without a HIP device bench.py says so instead of measuring something else."""
    import subprocess
    import sys

    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "needs a GPU" in (out.stderr + out.stdout)


def test_bench_refuses_arguments_it_cannot_honour():
    """--steps sets the number of timed steps (at least one); the score gather is one of --full's checks."""
    import subprocess
    import sys

    for extra in (["--steps", "0"], ["--warmup", "-1"], ["--gather"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 2 and "error:" in out.stderr, (extra, out.stderr)


def test_bench_dump_outputs_stays_within_its_size_limit(tmp_path):
    """bench.py --dump-outputs: float64 scores, the whole output while it fits the limit, else a fixed seeded sample with the
    sampled positions' indices beside it; the same scores give the same files."""
    import subprocess
    import sys

    script = (
        "import sys, torch, bench\n"
        "bench.DUMP_LIMIT_BYTES = 4096\n"
        "d = sys.argv[1]\n"
        "bench.dump_outputs(d + '/small', 'scores', torch.arange(-256, 256, dtype=torch.int32), 0, 1)\n"
        "for run in ('a', 'b'):\n"
        "    bench.dump_outputs(d + '/' + run, 'scores', torch.arange(100000, dtype=torch.int32) * 7 - 5, 0, 1)\n"
        "bench.dump_outputs(d + '/ranks', 'scores', torch.arange(100000, dtype=torch.int32), 1, 2)\n")
    subprocess.check_call([sys.executable, "-c", script, str(tmp_path)], cwd=ROOT, timeout=300)
    small = np.load(tmp_path / "small" / "scores.npy")
    assert small.dtype == np.float64 and np.array_equal(small, np.arange(-256, 256))
    assert sorted(os.listdir(tmp_path / "a")) == ["scores.npy", "scores_index.npy"]
    scores, index = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "a" / "scores_index.npy")
    assert scores.dtype == index.dtype == np.float64 and 0 < scores.size == index.size <= 4096 // 16
    assert np.all(np.diff(index) > 0) and np.array_equal(scores, index * 7 - 5)
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 4096
    assert np.array_equal(scores, np.load(tmp_path / "b" / "scores.npy"))
    assert sorted(os.listdir(tmp_path / "ranks")) == ["scores_rank1.npy", "scores_rank1_index.npy"]
    assert np.load(tmp_path / "ranks" / "scores_rank1.npy").size <= 4096 // 2 // 16


def test_cpp_mirror_reports_the_missing_device_as_an_exception(tmp_path):
    """spx_nnue::NnueState on a box without a GPU: the library's SPX_ERR_NO_DEVICE surfaces as spx_nnue::Error (the
    reference's calls cannot fail; the mirror must not pretend to evaluate)."""
    import subprocess

    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    src = tmp_path / "t.cpp"
    src.write_text('#include "spx_nnue.hpp"\n#include <cstdio>\n'
                   'int main() { try { auto net = spx_nnue::Network::synthetic(0); spx_nnue::NnueState st(net); }\n'
                   '  catch (const spx_nnue::Error& e) { std::printf("%d %s\\n", e.status, e.what()); return 0; }\n'
                   '  return 1; }\n')
    exe = tmp_path / "t"
    lib_dir = os.path.join(ROOT, "stormphrax_amd")
    # (Network::synthetic: the dev build of the library and the mirror's SPX_NNUE_DEV part)
    subprocess.check_call(["g++", "-std=c++17", "-DSPX_NNUE_DEV", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lspx_nnue_dev", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("4 "), out.stdout + out.stderr
    assert "no CPU fallback" in out.stdout
