"""SharedMap of the header-only C++17 facade (include/beluga_amd/amcl.hpp): tests/cpp/shared_map_demo.cpp compiles with plain g++ -Werror
against the C ABI, as the programs of test_cpp_facade.py do, and - on a GPU - runs three batch members on one shared map beside lone
twins that hold the grid privately."""
import os
import subprocess

import pytest

from beluga_amd import build as mcl_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    mcl_build.build()
    exe = tmp_path_factory.mktemp("cpp") / "shared_map_demo"
    lib_dir = os.path.join(ROOT, "beluga_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shared_map_demo.cpp"), "-L", lib_dir, "-lbeluga_mcl",
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
def test_members_on_a_shared_map_equal_their_twins_and_outlive_the_handle(demo):
    out = subprocess.run([demo], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [line.split() for line in out.stdout.splitlines()]
    kv = {l[0]: l[1:] for l in lines if l[0] != "particles"}
    assert kv["members"] == ["3"] and kv["equal"] == ["1"]
    assert kv["cycles"] == ["4"] and kv["kernel_launches"] == ["12"]
    assert kv["members_fused"] == ["12"] and kv["members_alone"] == ["0"]
    assert kv["users"] == ["3", "3"] and int(kv["map_bytes"][0]) > 15 * 101 * 75
    assert kv["shared_members"] == ["3"] and kv["owned_bytes"] == ["0"]
    sizes = {int(l[1]): int(l[2]) for l in lines if l[0] == "particles"}
    assert sizes[0] == 300 and 200 <= sizes[1] <= 900 and sizes[2] == 1025
