"""CPU: the bookkeeping of the engine's Winograd-transform cache (csrc/lip_bindcache.h), driven by a stand-alone host
program with a counting allocator (tests/bind_cache_host.cpp): first use fills, the second finds; keys tell forms,
sources and geometries apart; a second stream gets nothing; the invalidation order of a primal pass (stale before its
launches and after them, refilled in place, the owning stream kept); the cap, a cap of zero, a failed allocation, a
failed fill; release on re-binding and destruction frees exactly what was allocated."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "laplace-inducing-points_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no C++ compiler found (set CXX)")


def test_bind_cache_bookkeeping(tmp_path):
    exe = tmp_path / "bind_cache_host"
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(HERE, "bind_cache_host.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "bind cache host check ok" in r.stdout
