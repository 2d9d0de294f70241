"""CPU: images.PinnedPairs, the ring of (left, right) buffers behind run_split and TrainLoader, on pageable memory."""
import numpy as np
import pytest
import torch

from stereo_rcnn_amd import images


class _Event(object):
    def __init__(self):
        self.waited = 0

    def synchronize(self):
        self.waited += 1


def test_pinned_pairs_ring(monkeypatch):
    """entry(j) and entry(j + n) are one entry; put() returns a view of the source's shape and bytes inside the entry's own
    buffer; a fixed ring refuses an image beyond its entries with run_split's message and a growing one takes it; entry() waits on
    a reader's event once and clears it."""
    allocated = []

    def pageable(nbytes):                                   # the allocation seam: no page-locking without a device
        allocated.append(nbytes)
        return torch.empty(nbytes, dtype=torch.uint8)
    monkeypatch.setattr(images, '_page_locked', pageable)
    rng = np.random.RandomState(0)
    small = rng.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    big = rng.randint(0, 256, (512, 1408 + 1, 3)).astype(np.uint8)            # one column beyond a fixed entry
    for grow, nbytes in ((False, 3 * 512 * 1408), (True, 3 * 376 * 1242)):
        ring = images.PinnedPairs(3, grow=grow)
        assert ring.entry(1) is ring.entry(4) is ring.entry(7) and ring.entry(1) is not ring.entry(2)
        e = ring.entry(4)
        assert e == [None, None, None] and not allocated                       # buffers come with the first put
        left = ring.put(e, 0, small)
        right = ring.put(e, 1, small[:, ::-1])                                 # a non-contiguous source
        assert allocated == [nbytes, nbytes]
        assert left.dtype == torch.uint8 and tuple(left.shape) == small.shape and np.array_equal(left.numpy(), small)
        assert np.array_equal(right.numpy(), small[:, ::-1])
        assert left.data_ptr() == e[0].data_ptr() and right.data_ptr() == e[1].data_ptr()
        assert ring.put(e, 0, small + 1).data_ptr() == e[0].data_ptr() and allocated == [nbytes, nbytes]    # reused, not reallocated
        if grow:
            view = ring.put(e, 0, big)
            assert allocated[2:] == [big.nbytes] and np.array_equal(view.numpy(), big) and view.data_ptr() == e[0].data_ptr()
            assert np.array_equal(ring.put(e, 0, small).numpy(), small) and len(allocated) == 3              # stays grown
        else:
            with pytest.raises(AssertionError, match="image larger than the staging ring's entries"):
                ring.put(e, 0, big)
            with pytest.raises(AssertionError, match="image larger than the staging ring's entries"):
                ring.put(ring.entry(2), 0, big)                                # nor into an entry without a buffer yet
            assert len(allocated) == 2
        ev = _Event()
        e[2] = ev
        assert ring.entry(0) is not e and ev.waited == 0                      # another entry's reader is not waited for
        assert ring.entry(7) is e and ev.waited == 1 and e[2] is None
        assert ring.entry(4) is e and ev.waited == 1
        del allocated[:]
