"""The host side of the batch-free device entries (device_calls.py) without a GPU: the grow-and-repeat protocol against a
stand-in call, and that HipEngine still offers every method under its name."""
import pytest
import torch

from squarna_amd import device_calls as D, engine as E


class _Call:
    """A stand-in entry: `total` records 0, 1, ... exist; it writes those that fit, counts them all, reports `status`."""

    def __init__(self, total, status=0):
        self.total, self.status, self.caps = total, status, []

    def __call__(self, tensors, cap, out):
        self.caps.append(cap)
        assert [int(t.numel()) for t in tensors] == [cap, cap] and out.tolist() == [0, 0]
        k = min(cap, self.total)
        tensors[0][:k] = torch.arange(k, dtype=torch.int64)
        tensors[1][:k] = torch.arange(k, dtype=torch.int32) * 2
        out[0], out[1] = self.total, self.status


def _run(call, cap):
    return D._call_until_fits(torch.device("cpu"), cap, (torch.int64, torch.int32), call, "a status was reported")


def test_one_call_when_the_buffers_suffice():
    call = _Call(5)
    a, b = _run(call, 8)
    assert call.caps == [8] and a.tolist() == list(range(5)) and b.tolist() == list(range(0, 10, 2))
    assert (a.dtype, b.dtype) == (torch.int64, torch.int32)


def test_one_repeat_with_the_true_number():
    call = _Call(10)
    a, b = _run(call, 4)
    assert call.caps == [4, 10]                                              # repeated once, with the number the call reported
    assert a.tolist() == list(range(10)) and b.tolist() == list(range(0, 20, 2))


def test_exactly_full_is_not_repeated_and_none_is_empty():
    call = _Call(4)
    assert _run(call, 4)[0].tolist() == [0, 1, 2, 3] and call.caps == [4]
    call = _Call(0)
    assert [int(t.numel()) for t in _run(call, 4)] == [0, 0] and call.caps == [4]


def test_a_status_raises_before_any_repeat():
    call = _Call(10, status=2)
    with pytest.raises(RuntimeError, match="a status was reported"):
        _run(call, 4)
    assert call.caps == [4]


def test_the_engine_still_offers_the_device_methods():
    names = ("matrix_select", "matrix_cells", "first_fit", "align_pair_count", "window_pair_count", "score_tensors", "_pow17_table")
    assert issubclass(E.HipEngine, D.DeviceCalls)
    for name in names:
        assert getattr(E.HipEngine, name) is getattr(D.DeviceCalls, name) and name not in vars(E.HipEngine)
    assert E._upload_once is D._upload_once and E._TABLES[0] == "partner"
    eng = E.HipEngine()
    assert eng._pow17_table(3).tolist() == [(0.5 * k) ** 1.7 for k in range(13)] and len(eng._pow17) == 4 * 64 + 1
    assert E.HipEngine()._pow17 is None                                      # (the table is the engine's own)
