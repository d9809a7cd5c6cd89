"""The tile kernel's lookup-free slots (csrc/tile_step_kernel.h: make_tile_head / ts_head_tile) against the host-built map,
which stays the truth.  Host code only: compiled with hipcc and run here, no GPU.  Every slot the plan calls regular decodes
to exactly its map entry, every other slot is resolved by the lookup, the headline shape has all its 228 whole layer-0 tiles
regular, and a plan whose decode disagrees with the map in one slot reports "not regular" and sends every slot to the lookup."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tile_head_check.hip")
SHAPES = [[784, 300, 100, 10], [784, 100, 50, 10], [300, 40, 10], [100, 64, 48, 32, 10], [1000, 512, 256, 16], [200, 48, 10]]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("tile_head") / "tile_head_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", out, SRC], check=True, capture_output=True, timeout=600)
    return out


def run(checker, cus, dims, force=False):
    r = subprocess.run([checker, str(cus), "1" if force else "0"] + [str(d) for d in dims], check=True, capture_output=True, text=True, timeout=60)
    out = {}
    for line in r.stdout.strip().splitlines():
        f = line.split()
        out[f[0]] = dict(zip(f[1::2], map(int, f[2::2])))
    assert set(out) == {"full", "first"}
    return out


@pytest.mark.parametrize("dims", SHAPES)
def test_regular_slots_decode_to_their_map_entries(checker, dims):
    for name, m in run(checker, 32, dims).items():     # the map of all layers and the forward-only map
        assert m["mismatches"] == 0 and m["unresolved"] == 0, name
        assert m["whole"] > 0, name
        if dims[0] == 1000:
            # 644 tiles on 256 CUs: more than 15 slots in front of an XCD's rectangle order (whole layer-0 tiles among them),
            # which the four bits per XCD cannot name -- the plan says so and every slot takes the lookup
            assert m["plan_regular"] == 0 and m["regular"] == 0, name
        else:
            assert m["plan_regular"] == 1, name
            assert m["regular"] >= m["whole_regular"] == m["whole"], name   # every whole layer-0 tile is decoded, none looked up


def test_headline_shape_has_every_whole_layer0_tile_regular(checker):
    out = run(checker, 32, [784, 300, 100, 10])
    assert out["full"]["grid"] == 288
    for m in out.values():
        assert m["whole"] == 228 and m["whole_regular"] == 228 and m["regular"] == 228


def test_clipped_rectangle_and_partial_last_row(checker):
    # 208 x 48 padded: 3 tile columns over rectangles 2 wide (the second one clipped to 1), 3 whole tile rows over 4 rows of
    # rectangles (the last of them past the edge), and a last tile row of 16 weights that is looked up
    out = run(checker, 32, [200, 48, 10])
    for m in out.values():
        assert m["whole"] == 9 and m["regular"] == 9 and m["mismatches"] == 0 and m["unresolved"] == 0


@pytest.mark.parametrize("dims", [[784, 300, 100, 10], [200, 48, 10]])
def test_a_decode_that_disagrees_with_the_map_turns_the_plan_off(checker, dims):
    for name, m in run(checker, 32, dims, force=True).items():
        assert m["plan_regular"] == 0 and m["regular"] == 0, name
        assert m["unresolved"] == 0, name               # every slot by lookup
