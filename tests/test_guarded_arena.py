"""The guarded arena (tests/guarded_arena.py) itself, on the CPU: torch-only fake "kernels" on a CPU arena.  A correct one passes; one
that stores a single element past a frame, behind an item or into a source, leaves a pixel unwritten or consumes a guard value raises
GuardError, and the message names the block and the coordinates.  The guarded GPU tests (tests/test_gpu_guarded_motion.py) are worth
what these are worth."""
import pytest
import torch

from tests.guarded_arena import G, GAP, POISON, Arena, GuardError, Plain, assert_bit_identical, bstride

H, W, C, NB = 5, 7, 8, 3


def _case(al):
    """A fat source and destination (fp16 NHWC), a thin source and destination, nb = 3 flat items in and out (a batched launch)."""
    torch.manual_seed(3)
    b = dict(fs=al.fat(2, H, W, C, torch.float16, name='fs'), fd=al.fat(2, H, W, C, torch.float16, name='fd'),
             ts=al.thin(2, H, W, name='ts'), td=al.thin(2, H, W, name='td'),
             xs=al.flat(NB, (10,), torch.float32, name='xs'), xd=al.flat(NB, (10,), torch.float32, name='xd'),
             ws=al.flat(1, (5,), torch.int64, zero=True, name='ws'))
    al.fill(b['fs'], torch.randn(2, H, W, C))
    al.fill(b['ts'], torch.randn(2, H, W))
    al.fill(b['xs'], torch.randn(NB, 10))
    return b


def _kernel(b):
    """The correct fake: every destination element from its source element, nothing else touched."""
    b['fd'].copy_(b['fs'] * 2)
    b['td'].copy_(b['ts'] + 1)
    b['xd'].copy_(-b['xs'])


def _byte(al, t, elements):
    """Index into the slab of the byte `elements` elements behind (in front of, if negative) the first element of t."""
    return t.data_ptr() - al.slab.data_ptr() + elements * t.element_size()


def _run(sabotage=None, written=('fd', 'td', 'xd')):
    al = Arena('cpu', 1 << 20)
    b = _case(al)
    al.snapshot()
    _kernel(b)
    if sabotage is not None:
        sabotage(al, b)
    w = [b[k] for k in written]
    al.check(w)
    al.assert_finite(w)
    al.record(w)
    return al, b


def test_layout_is_pitched_guarded_and_poisoned():
    al = Arena('cpu', 1 << 20)
    b = _case(al)
    fd, td, xd, ws = b['fd'], b['td'], b['xd'], b['ws']
    assert fd.shape == (2, H, W, C) and fd.stride() == ((H + 2 * G) * (W + 2 * G) * C, (W + 2 * G) * C, C, 1)
    assert td.shape == (2, H, W) and td.stride() == ((H + 2 * G) * (W + 2 * G), W + 2 * G, 1)
    assert xd.shape == (NB, 10) and bstride(xd) == 256 + GAP and bstride(xd) != 40 and xd[1].is_contiguous()
    assert int(ws.count_nonzero()) == 0 and ws.numel() * 8 == 40
    assert int(al.slab[_byte(al, ws, 5)]) == POISON                     # the poison starts at byte workspace_bytes
    assert bool(torch.isnan(fd).all()) and bool(torch.isnan(td).all()) and bool(torch.isnan(xd).all())      # poisoned until written
    n4 = al.thin(3, H, W, n=2)
    assert n4.shape == (2, 3, H, W) and bstride(n4) == 3 * (H + 2 * G) * (W + 2 * G) * 4
    # every byte that is not inside a written frame or item is poison: guards, gaps, the space between two blocks
    live = torch.zeros_like(al.slab)
    for t in (b['fs'], b['ts'], b['xs'], ws):
        al._like(live, t).view(torch.uint8 if t.element_size() == 1 else {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).fill_(-1)
    assert bool((al.slab[live == 0] == POISON).all()) and int((live != 0).sum()) == (2 * H * W * C) * 2 + 2 * H * W * 4 + NB * 40 + 40
    for a_, b_ in zip(al._blocks, al._blocks[1:]):
        assert b_.off - (a_.off + a_.nbytes) >= GAP and bool((al.slab[a_.off + a_.nbytes:b_.off] == POISON).all())
    assert al._blocks[0].off >= GAP


def test_a_correct_kernel_passes_and_matches_the_plain_run():
    al, b = _run()
    assert torch.equal(b['fd'], b['fs'] * 2) and torch.equal(b['xd'], -b['xs'])
    pl = Plain('cpu')
    pb = _case(pl)
    _kernel(pb)
    w = [pb[k] for k in ('fd', 'td', 'xd')]
    pl.assert_finite(w)
    pl.record(w)
    assert_bit_identical(al, pl)
    pl.bits[1][0, 0, 0] += 1
    with pytest.raises(GuardError, match=r'written region 1 differs from the plain run at \[0, 0, 0\]'):
        assert_bit_identical(al, pl)


def test_store_at_column_W_of_a_fat_view_raises():
    def sab(al, b):
        al.slab[_byte(al, b['fd'][1, 2], W * C + 3)] = 0                 # image 1, row 2, column W, channel 3
    with pytest.raises(GuardError, match=r'"fd".*column 7 \(= W\) of image 1 written, at \(image 1, row 2, column 7, channel 3\)'):
        _run(sab)


def test_store_at_row_minus_one_of_a_thin_plane_raises():
    def sab(al, b):
        al.slab[_byte(al, b['td'][1], -(W + 2 * G) + 4)] = 0             # plane 1, row -1, column 4
    with pytest.raises(GuardError, match=r'"td".*row -1 of plane 1 written, at \(plane 1, row -1, column 4, channel 0\)'):
        _run(sab)


def test_store_one_byte_behind_a_flat_item_raises():
    def sab(al, b):
        al.slab[_byte(al, b['xd'][NB - 1], 10)] = 0                      # element 10 of the last item: the first byte behind the block
    with pytest.raises(GuardError, match=r'guard bytes between two blocks written, 0 bytes behind block \d+ "xd"'):
        _run(sab)
    def ws(al, b):
        al.slab[_byte(al, b['ws'], 5)] = 0                               # byte workspace_bytes of a workspace
    with pytest.raises(GuardError, match=r'0 bytes behind block \d+ "ws"'):
        _run(ws)


def test_store_into_the_gap_between_two_batched_items_raises():
    def sab(al, b):
        al.slab[_byte(al, b['xd'][1], 10) + 2] = 0                       # 2 bytes behind item 1, in front of item 2
    with pytest.raises(GuardError, match=r'"xd".*byte 2 behind item 1 written \(the gap between item 1 and item 2\)'):
        _run(sab)


def test_a_modified_source_interior_raises():
    def sab(al, b):
        b['fs'][0, 4, 6, 7] += 1
    with pytest.raises(GuardError, match=r'"fs".*source interior written at \(image 0, row 4, column 6, channel 7\)'):
        _run(sab)
    def flat(al, b):
        b['xs'][2, 9] += 1
    with pytest.raises(GuardError, match=r'"xs".*source interior written at \(item 2, byte 36, element 9\)'):
        _run(flat)
    def zero(al, b):
        b['ws'][0, 4] = 1                                                  # a workspace that is not left all-zero
    with pytest.raises(GuardError, match=r'"ws".*source interior written at \(item 0, byte 32, element 4\)'):
        _run(zero)
    # a destination whose other channels the launch does not own
    al = Arena('cpu', 1 << 20)
    b = _case(al)
    al.snapshot()
    b['fd'].copy_(b['fs'])
    with pytest.raises(GuardError, match=r'"fd".*a part of a destination that the launch does not own written at \(image 0, row 0, column 0, channel 4\)'):
        al.check([b['fd'][..., :4], b['td'], b['xd']])


def test_an_unwritten_output_pixel_raises():
    def sab(al, b):
        al.poison(b['td'][1, 3, 5:6])
    with pytest.raises(GuardError, match=r'"td".*nan at index \[1, 3, 5\] of the written region .* never written \(1 of'):
        _run(sab)


def test_a_consumed_guard_value_raises():
    def sab(al, b):
        # a clamp that is off by one: the last column of the output reads column W of the source
        wide = torch.as_strided(b['fs'], (2, H, W + 1, C), b['fs'].stride(), b['fs'].storage_offset())
        b['fd'][:, :, W - 1] = wide[:, :, W] * 2
    with pytest.raises(GuardError, match=r'"fd".*nan at index \[0, 0, 6, 0\].*a poisoned value was consumed'):
        _run(sab)


def test_check_needs_a_snapshot_and_foreign_tensors_are_refused():
    al = Arena('cpu', 1 << 20)
    with pytest.raises(AssertionError):
        al.check([])
    with pytest.raises(AssertionError):
        al.fill(torch.zeros(4), torch.ones(4))
    with pytest.raises(MemoryError):
        al.flat(1, (2 << 20,), torch.uint8)
