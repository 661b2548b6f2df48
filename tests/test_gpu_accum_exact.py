"""The batch launch's cursor offset (csrc/kernels/api.h AugArgs::cursor_off), bit for bit: the K
batch launches of an accumulated step share one device cursor, which the step's last launch
advances by K, and read it at offsets 0..K-1 baked into the captured graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def test_augment_cursor_offset(native_ext):
    """AugArgs::cursor_off: B 4, L 10, device cursor 1, offsets 0..2 -- positions 4..7, 8..11 and
    12..15 mod 10, so offsets 1 and 2 wrap -- against a launch whose cursor holds cur + off and
    whose offset is 0: x and y bit for bit. The offset launch leaves the cursor alone."""
    from ddp_amd.data import DeviceLoader, SyntheticCIFAR10
    ld = DeviceLoader(SyntheticCIFAR10(True, n=10), 4, DEV)
    assert ld.idx.numel() == 10
    got = {}
    for off in range(3):
        ld.cursor.fill_(1)
        x, y = ld.fill(advance=False, offset=off)
        torch.cuda.synchronize()
        assert int(ld.cursor) == 1
        got[off] = (x.clone(), y.clone())
    for off in range(3):
        ld.cursor.fill_(1 + off)
        x, y = ld.fill(advance=False)
        torch.cuda.synchronize()
        assert torch.equal(x.view(torch.int16), got[off][0].view(torch.int16)), off
        assert torch.equal(y, got[off][1]), off
    # the three batches differ (a launch that ignored the offset would pass the loop above
    # only if it also ignored the cursor)
    assert not torch.equal(got[0][1], got[1][1]) or not torch.equal(got[0][0], got[1][0])
    want = ld.labels[ld.idx[torch.arange(12, 16) % 10].long()].long()
    assert torch.equal(got[2][1], want)
    assert ld.cursor_advance(3) == (ld.cursor.data_ptr(), 3)
