"""estimate_clusters() and cluster_labels() of the header-only C++17 facade (include/beluga_amd/amcl.hpp): tests/cpp/cluster_modes_demo.cpp
compiles with plain g++ -Werror against the C ABI, as the programs of test_cpp_facade.py do, and - on a GPU - finds the four peaks of
the reference's fine multicluster set."""
import os
import subprocess

import pytest

from beluga_amd import build as mcl_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    mcl_build.build()
    exe = tmp_path_factory.mktemp("cpp") / "cluster_modes_demo"
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cluster_modes_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl",
                           f"-Wl,-rpath,{lib_dir}", "-o", str(exe)])
    return str(exe)


def test_demo_compiles_and_never_answers_without_a_gpu(demo):
    import torch
    out = subprocess.run([demo], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert out.returncode == 0, out.stdout + out.stderr
    else:  # no CPU fallback: the constructor throws
        assert out.returncode == 3 and "no CPU fallback" in out.stdout


@pytest.mark.gpu
def test_facade_finds_the_four_peaks(demo):
    out = subprocess.run([demo], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    kv = {l[0]: l[1:] for l in lines}
    n = int(kv["particles"][0])
    assert n == 25_600 and kv["clusters"] == ["4"] and kv["two"] == ["2"]
    entries = [(int(l[1]), int(l[2])) + tuple(float(v) for v in l[3:]) for l in lines if l[0] == "entry"]
    assert len(entries) == 4
    weights = [e[2] for e in entries]
    assert weights == sorted(weights, reverse=True) and weights[-1] > 0.0
    assert sorted(e[0] for e in entries) == [0, 1, 2, 3] and all(e[1] > 1 for e in entries)
    # one peak per quadrant, the heaviest where both coordinates are positive (HeaviestClusterSelectionTest :357-386)
    assert sorted((e[3] > 0, e[4] > 0) for e in entries) == [(False, False), (False, True), (True, False), (True, True)]
    assert entries[0][3] > 0 and entries[0][4] > 0
    assert all(0.0 < e[5] < 1.0 and 0.0 < e[6] < 1.0 for e in entries)  # variances of a cluster inside its quadrant
    best = [float(v) for v in kv["cluster_based_estimate"]]
    assert abs(best[0] - entries[0][3]) < 1e-9 and abs(best[1] - entries[0][4]) < 1e-9
    # labels: one per particle, all in range, and as many of each as the entry counts
    assert kv["labels"] == [str(n), "0"]
    counts = {int(l[1]): int(l[2]) for l in lines if l[0] == "label_count"}
    assert counts == {e[0]: e[1] for e in entries} and sum(counts.values()) == n
