"""GPU: what `_lib.launch` can only refuse with device tensors at hand -- a tensor that is not contiguous, a tensor on another
device than the launch's.  Both are GcfrErrors before the entry is called (the entry is replaced by a function that fails the
test if it is reached), so nothing faulty ever reaches the device."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _reached(*a, **k):
    raise AssertionError("a refused call reached the entry")


def _rig_fwd_args(device, final=None):
    from geomconsistentfr_amd import _lib
    B, L, H, W = 1, 1, 4, 4
    z = lambda *s: torch.zeros(*s, device=device)
    final = z(B, L, H, W) if final is None else final
    return (final, z(B, 3, H, W), z(1, L, 3), 1, B, L, H, W, z(B, 3, H, W), z(B, 3, H, W), _lib.STREAM)


def test_launch_refuses_a_tensor_that_is_not_contiguous(monkeypatch):
    from geomconsistentfr_amd import _lib
    monkeypatch.setattr(_lib.load(), "gcfr_light_rig_fwd", _reached)
    transposed = torch.arange(16.0, device=DEV).reshape(4, 4).t()
    assert transposed.dtype == torch.float32 and not transposed.is_contiguous()
    with pytest.raises(_lib.GcfrError, match="gcfr_light_rig_fwd.*not contiguous"):
        _lib.launch("gcfr_light_rig_fwd", DEV, *_rig_fwd_args(DEV, final=transposed))


def test_launch_refuses_a_tensor_on_another_device(monkeypatch):
    from geomconsistentfr_amd import _lib
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    monkeypatch.setattr(_lib.load(), "gcfr_light_rig_fwd", _reached)
    other = torch.zeros(1, 1, 4, 4, device="cuda:1")
    with pytest.raises(_lib.GcfrError, match="gcfr_light_rig_fwd.*cuda:1"):
        _lib.launch("gcfr_light_rig_fwd", DEV, *_rig_fwd_args(DEV, final=other))
