"""The integer arithmetic of the 384 x 192 one-per-CU launches (peneo_amd/csrc/gemm_walk.h: XCD order, grouped tile walk, pieces of
a ragged last k-tile) checked on the CPU: tests/host/gemm_walk_check.cpp includes the header the kernels include, is built here as
a stand-alone program with the address and undefined-behaviour sanitizers, and run.  It walks every tile of the groups of
test_gpu_gemm_group_nn384.py and of an encoder layer's four weight gradients: each tile exactly once, and ceil(rem / 8) pieces in a tail."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_walk_host_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemm_walk_check")
    src = os.path.join(ROOT, "tests", "host", "gemm_walk_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "gemm_walk_check: ok" in run.stdout
