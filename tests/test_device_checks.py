"""CPU: the host layer's one tensor check (ptmi.device._check_tensor), over every
buffer kind the host layer accepts. No GPU here, so every tensor offered is
wrong at least by its device; each row is offered a non-tensor, a wrong dtype,
a wrong shape, a non-contiguous view and a CPU tensor that is right otherwise,
and each must be a PtmiError that begins with the argument's name."""
import numpy as np
import pytest
import torch

from ptmi import _lib, device

H, W = 3, 5
DEV = torch.device('cuda', 0)
f32, i32 = torch.float32, torch.int32

# name, shape, dtype, a wrong dtype, a wrong shape
KINDS = [('accum', (H, W, 3), f32, torch.float64, (H, W, 4)),
         ('stats', (H, W, 4), f32, torch.float16, (H, W, 3)),
         ('guides', (H, W, 8), f32, i32, (H, W, 4)),
         ('ids', (H, W), i32, torch.int64, (H, W, 1)),
         ('var', (H, W), f32, i32, (W, H)),
         ('tiles', (7,), i32, f32, (7, 1))]


def offers(shape, dtype, wrong_dtype, wrong_shape):
    wide = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype)
    return {'a non-tensor': np.zeros(shape, np.float32),
            'a wrong dtype': torch.zeros(shape, dtype=wrong_dtype),
            'a wrong shape': torch.zeros(wrong_shape, dtype=dtype),
            'a non-contiguous view': wide[..., ::2],
            'a CPU tensor': torch.zeros(shape, dtype=dtype)}


def check(name, t, shape, dtype):
    if name == 'tiles':  # the tile list goes through its own entry: a 1-D list of any length, with a count
        return device._check_tiles((t, 2), DEV)
    kinds = device.Integrator.IMAGE_KINDS
    assert (H, W) + kinds[name][0] == shape and kinds[name][1] == dtype  # the table the integrator checks by
    return device._check_tensor(name, t, shape, dtype, DEV)


@pytest.mark.parametrize('name,shape,dtype,wrong_dtype,wrong_shape', KINDS, ids=[k[0] for k in KINDS])
def test_every_buffer_kind_is_checked(name, shape, dtype, wrong_dtype, wrong_shape):
    for what, t in offers(shape, dtype, wrong_dtype, wrong_shape).items():
        if isinstance(t, torch.Tensor) and what != 'a non-contiguous view':
            assert t.is_contiguous()
        if what == 'a non-contiguous view':
            assert tuple(t.shape) == shape and t.dtype == dtype and not t.is_contiguous()
        with pytest.raises(_lib.PtmiError) as e:
            check(name, t, shape, dtype)
        assert str(e.value).startswith(f'{name} must be a contiguous '), (what, str(e.value))


def test_no_tiles_is_the_whole_frame():
    assert device._check_tiles(None, DEV) == (None, 0)


def test_a_named_size_matches_any_size_and_is_named_in_the_message():
    with pytest.raises(_lib.PtmiError, match=r'accum must be a contiguous cuda float32 tensor of shape \(H, W, 3\)'):
        device._check_tensor('accum', torch.zeros((H, W, 3)), ('H', 'W', 3), f32, DEV)
