"""vers_amd/host/ivfflat.hpp's fetch and search_by_id from compiled code (tests/cpp/fetch_demo.cpp), linked against the library these tests
run against, as tests/test_update_cpp_gpu.py does for update_batch."""
import os
import subprocess

import pytest

from vers_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_host_mirror_fetch_and_search_by_id(tmp_path):
    lib = capi.LIB_PATH
    exe = str(tmp_path / "fetch_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fetch_demo.cpp"),
                           "-L" + os.path.dirname(lib), "-lvers_hip", "-Wl,-rpath," + os.path.dirname(lib)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "SAME" in out.stdout, out.stdout + out.stderr
