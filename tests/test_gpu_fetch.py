"""upload.PinnedFetch on the GPU: the device -> host fetches of the epoch
loops (run_epoch's loss + probabilities, score_epoch's loss + counts)."""
import pytest

pytestmark = pytest.mark.gpu


def test_pinned_fetch_keeps_one_batch_in_flight_and_reuses_its_buffers():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
    from ggnn_amd.upload import PinnedFetch
    dev = torch.device("cuda")

    def batch(k):
        """A 0-dim loss, 8 floats as [2, 4] and 5 int32, all depending on k."""
        return [torch.tensor(float(k), device=dev), torch.arange(8, dtype=torch.float32, device=dev).reshape(2, 4) + k,
                torch.arange(5, dtype=torch.int32, device=dev) * k]

    def holds(host, tensors):
        return all(h.device.type == "cpu" and h.shape == t.shape and h.dtype == t.dtype and torch.equal(h, t.cpu())
                   for h, t in zip(host, tensors)) and len(host) == len(tensors)

    ptrs = lambda host: [h.data_ptr() for h in host]
    f = PinnedFetch()
    a, b = batch(1), batch(2)
    host_a, ev_a = f.fetch(a)
    host_b, ev_b = f.fetch(b)
    ev_a.synchronize()
    ev_b.synchronize()
    # the batch in flight: B's fetch left A's host views alone
    assert holds(host_a, a) and holds(host_b, b)
    assert not set(ptrs(host_a)) & set(ptrs(host_b))
    assert host_a[0].is_pinned() and host_b[0].is_pinned()
    # the third fetch takes the first set's storage again
    c = batch(3)
    host_c, ev_c = f.fetch(c)
    ev_c.synchronize()
    assert ptrs(host_c) == ptrs(host_a)
    assert holds(host_c, c) and holds(host_b, b)
    # the second set again: slot 0 as before, a larger tensor in slot 1 and
    # another dtype in slot 2 get fresh buffers
    d = [b[0], torch.arange(16, dtype=torch.float32, device=dev) + 4, torch.arange(5, dtype=torch.float32, device=dev)]
    host_d, ev_d = f.fetch(d)
    ev_d.synchronize()
    assert host_d[0].data_ptr() == host_b[0].data_ptr()
    assert host_d[1].data_ptr() != host_b[1].data_ptr() and host_d[2].data_ptr() != host_b[2].data_ptr()
    assert holds(host_d, d) and holds(host_c, c)
    assert all(h.is_pinned() for h in host_d)
