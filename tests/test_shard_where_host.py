"""The "where" round of the sharded fetch / update / search by id on the HOST: tests/cpp/shard_where_demo.cpp builds
vers_amd/csrc/shard_where.hpp with the host compiler alone (AddressSanitizer + UBSan, a stand-alone program) -- the agreement on the first
failing rank's status, the claimer and cluster per request, a double claim, a claim by a rank that does not own the list, the row round's
per-chunk per-rank counts, pad, callback count and slots at chunk sizes 1, 64 and n, an all-empty chunk, repeated ids, and that what a rank
packs at place p is what the placing kernel reads at that slot."""
import os
import subprocess

from tests.test_compact_kernel_host import host_clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_where_round_decisions_on_the_host(tmp_path):
    cxx = host_clang() or "c++"
    exe = str(tmp_path / "shard_where_demo")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "vers_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "shard_where_demo.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "all ok" in r.stdout, r.stdout + r.stderr
