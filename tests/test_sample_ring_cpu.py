"""csrc/sample_ring.h: what the worker threads that draw a sampled loop's batches share with the thread that uploads them and
enqueues the steps -- one sampler per group member, up to 8 threads.  Host code only: tests/native/sample_ring_check.cpp, a
stand-alone program, is built with g++ -fsanitize=thread and once more plainly, and run here, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sample_ring_check.cpp")
INC = os.path.join(ROOT, "graph-neural-net_amd", "csrc")


@pytest.mark.parametrize("sanitize", [True, False])
def test_chunks_handed_over_once_in_order(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path / "sample_ring_check")
    flags = ["-fsanitize=thread", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-I", INC] + flags + ["-o", out, SRC], check=True,
                   capture_output=True, timeout=300)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "sample ring ok"
    assert "ThreadSanitizer" not in r.stderr
