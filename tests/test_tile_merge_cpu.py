"""make_merged_tile_map (csrc/tile_step_kernel.h): the map in which the light tiles of the tile kernel's training launch share
workgroups -- groups of layer 0's partial last tile row, pairs of a later layer -- so that no CU runs two workgroups.
Host code only: compiled with hipcc and run here, no GPU.  Every tile of every layer is owned by exactly one workgroup,
a unit never leaves its tile row or its layer, pairs start at even columns, "usable" means no XCD holds more entries than it
has CUs, the headline shape gives 255 entries in a grid of 256, 1000-512-256-16 stays on the one-tile-per-workgroup map, and
make_tile_head validates on the merged map slot by slot."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tile_merge_check.hip")
SHAPES = [[784, 300, 100, 10], [784, 100, 50, 10], [80, 112, 48, 10], [96, 48, 32, 10], [100, 64, 48, 32, 10], [1000, 512, 256, 16]]
CUS = 32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("tile_merge") / "tile_merge_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", out, SRC], check=True, capture_output=True, timeout=600)
    return out


def run(checker, dims, cus=CUS):
    r = subprocess.run([checker, str(cus)] + [str(d) for d in dims], check=True, capture_output=True, text=True, timeout=60)
    f = r.stdout.split()
    return dict(zip(f[0::2], map(int, f[1::2])))


@pytest.mark.parametrize("dims", SHAPES)
def test_every_tile_has_exactly_one_owner(checker, dims):
    m = run(checker, dims)
    assert m["owned"] == m["expected"] and m["multiply_owned"] == 0
    assert m["out_of_layer"] == 0                    # no unit crosses a tile row or a layer
    assert m["odd_pairs"] == 0                       # a later layer's units start at even columns
    assert m["grid"] % 8 == 0 and m["live"] == m["whole"] + m["groups"] + m["pairs"] + m["singles"]
    assert m["usable"] == (m["max_xcd"] <= CUS)      # usable: no XCD holds more entries than it has CUs
    if m["usable"]:
        assert m["grid"] <= 8 * CUS and m["packed"] == 1


@pytest.mark.parametrize("dims", SHAPES)
def test_tile_head_validates_on_the_merged_map(checker, dims):
    m = run(checker, dims)
    assert m["mismatches"] == 0
    assert m["whole_not_first"] == 0                 # the whole layer-0 tiles come first in every XCD: no pair slots remain
    if m["whole"] and m["usable"]:
        assert m["plan_regular"] == 1 and m["regular"] == m["whole"]


def test_headline_shape_is_one_workgroup_per_cu(checker):
    m = run(checker, [784, 300, 100, 10])
    # 12 x 19 whole tiles, the 19 tiles of the 16-row last row in groups of 4, 4, 4, 4, 3, layer 1's 5 x 7 tiles in 5 x (2, 2, 2, 1),
    # layer 2's 2 x 1
    assert (m["whole"], m["groups"], m["pairs"], m["singles"]) == (228, 5, 15, 7)
    assert m["live"] == 255 and m["grid"] == 256 and m["usable"] == 1 and m["max_xcd"] == 32


def test_large_net_stays_on_the_one_tile_map(checker):
    m = run(checker, [1000, 512, 256, 16])
    assert m["usable"] == 0 and m["max_xcd"] > CUS


@pytest.mark.parametrize("dims,whole,groups", [([80, 112, 48, 10], 7, 2), ([96, 48, 32, 10], 3, 2), ([100, 64, 48, 32, 10], 8, 0)])
def test_partial_row_groups(checker, dims, whole, groups):
    # 80 = 64 + 16 rows: the last row's 7 columns in groups of 4 + 3; 96 = 64 + 32: 3 columns in groups of 2 + 1; 100 pads to
    # 112 = 64 + 48: a 48-row last tile row counts as whole (2 x 4 tiles), no group
    m = run(checker, dims)
    assert (m["whole"], m["groups"]) == (whole, groups)
    assert m["usable"] == 1
