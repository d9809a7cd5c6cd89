"""csrc/timer_slots.h: the slot accounting of the per-class kernel timers -- the cap of 8192 slots per class, reuse of the
created event pairs after a reset, launches of no class (cls < 0), events that cannot be created.  Host code only:
tests/native/timer_slots_check.cpp, a stand-alone program, is built with g++ and run here, no GPU -- with
-fsanitize=address,undefined, and once more plainly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "timer_slots_check.cpp")


@pytest.mark.parametrize("sanitize", [True, False])
def test_timer_slot_accounting(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path / "timer_slots_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", out, SRC], check=True, capture_output=True, timeout=300)
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "timer slots ok"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
