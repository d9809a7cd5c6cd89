"""NetGroup's argument checks that run before any device call, and its loud failure without a GPU."""
import numpy as np
import pytest


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_per_member_values():
    from gnn_amd import neural_net as nn
    assert np.array_equal(nn._per_member("steps", 0.5, 3), [0.5, 0.5, 0.5])
    assert np.array_equal(nn._per_member("steps", [0.1, 0.2], 2), [0.1, 0.2])
    assert np.array_equal(nn._per_member("momenta", np.array([0.9]), 1), [0.9])
    with pytest.raises(ValueError):
        nn._per_member("steps", [0.1, 0.2], 3)
    with pytest.raises(ValueError):
        nn._per_member("momenta", [], 1)


def test_wrong_lengths_are_refused_before_the_library_is_called(gnn):
    """A group object whose handle is null: a call that reached the library would return GNN_ERR_BAD_ARG (GnnError);
    a wrong-length steps / momenta sequence must raise ValueError first."""
    import ctypes as C
    g = gnn.NetGroup.__new__(gnn.NetGroup)
    g._lib, g._h, g.seeds, g.layer_dims, g.members = gnn.load_library(), C.c_void_p(), [1, 2, 3], [4, 3, 2], []
    with pytest.raises(ValueError):
        g.train_range(0, 8, 1, [0.1, 0.2], 0.9)
    with pytest.raises(ValueError):
        g.train_range(0, 8, 1, 0.1, [0.9] * 4)
    with pytest.raises(ValueError):
        g.train_sampled(None, 1, 8, 0.1, [0.9, 0.9])
    with pytest.raises(gnn.GnnError) as e:  # right lengths: the library refuses the null group
        g.train_range(0, 8, 1, 0.1, 0.9)
    assert e.value.code == 1


def test_group_without_gpu_fails_loudly(gnn):
    if _have_gpu():
        pytest.skip("GPU present")
    with pytest.raises(gnn.GnnError) as e:
        gnn.NetGroup([4, 3, 2], [1, 2])
    assert e.value.code == 4
