"""AmclBatch of the C++17 facade (include/beluga_amd/amcl.hpp) with members that return the cluster-based estimate, as the filter inside
beluga_amd::ros::Amcl does: tests/cpp/batch_cluster_demo.cpp compiles with plain g++ -Werror against the C ABI and - on a GPU - runs
four members for four cycles beside four lone filters made the same way."""
import os
import subprocess

import pytest

from beluga_amd import build as mcl_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    mcl_build.build()
    exe = tmp_path_factory.mktemp("cpp") / "batch_cluster_demo"
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "batch_cluster_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl",
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
def test_four_members_equal_four_lone_filters_and_share_two_cluster_launches(demo):
    out = subprocess.run([demo], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    estimates = [l for l in lines if l[0] == "estimate"]
    assert len(estimates) == 16 and {(int(l[1]), int(l[2])) for l in estimates} == {(c, i) for c in range(1, 5) for i in range(4)}
    kv = {l[0]: l[1:] for l in lines if l[0] != "estimate"}
    assert kv["members"] == ["4"] and kv["equal"] == ["1"]
    assert kv["cluster_launches"] == ["8"] and kv["members_cluster_fused"] == ["16"]
    assert kv["kernel_launches"] == ["12"]
    # the option off on every member: a fifth cycle that still equals the lone filters and does not move the cluster counter
    assert kv["equal_switched_off"] == ["1"] and kv["cluster_launches_switched_off"] == ["8"] and kv["members_fused"] == ["20"]
    assert kv["unknown_option_refused"] == ["1"]
