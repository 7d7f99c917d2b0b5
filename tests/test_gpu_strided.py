"""Pitched frames and sensor sub-rectangles through aqz_stage_append_strided.

Geometries, inputs and the layer-by-layer comparison are those of
test_gpu_kernel_matrix.py (imported): the smallest shapes that still have
interior regions plus ragged right and bottom edge regions.  Every device
source is a byte tensor sized tightly to the last byte of the last frame's
last row, and every byte outside the appended rectangles is poison (0xFF: NaN
for floats, nonzero for has_data), so a kernel that reads between rows, past
a row or past the rectangle either changes a pixel, sets a has_data flag of
the zero rows of _shallow2d's frame 2, or runs off the allocation.  Expected
layers and flags are expected_stage_layers on the packed frames; the route
(fused kernels reading in place / pack_frames first) is read from
aqz_stage_source_report.

Counts of the 2x2x2 group rule (G = 4 at z chunk 2, batches of 8): appends of
[8, 8] start at group boundaries with no pending plane, so all 16 frames are
whole groups read in place; [8, 3, 5] reads the first 8 in place, then 3 < G
frames go to the generic cascade (packed), which leaves 11 frames written --
not a group boundary -- so the last 5 go there too: 8 direct, 8 packed.
"""
from functools import lru_cache

import numpy as np
import pytest

from helpers import assert_same_pixels
from oracle_bindings import (DTYPE_NAMES, F32, F64, I8, I16, MEAN, METHOD_NAMES, MIN, SPACE, TIME,
                             U8, U16)
from test_gpu_kernel_matrix import (BPP, _case, _deep2d, _inputs, _name2d, _shallow2d, _vol,
                                    _xy2d, _xyvol)
from test_gpu_parity import KERNELS_3D, XY_KERNELS, XY_KERNELS_3D

pytestmark = pytest.mark.gpu
_ids = lambda d: DTYPE_NAMES[d]  # noqa: E731
POISON = 0xFF


def _canvas(c, pitch, frame_stride, off0):
    """Host bytes of c.frames (acquisition order) laid out pitched: pixel (0, 0)
    of frame 0 at byte off0, poison everywhere else, ending at the last byte of
    the last row."""
    n, h, w = c.frames.shape
    rb = w * BPP[c.dtype]
    size = off0 + (n - 1) * frame_stride + (h - 1) * pitch + rb
    buf = np.full(size, POISON, dtype=np.uint8)
    roi = np.lib.stride_tricks.as_strided(buf[off0:], shape=(n, h, rb),
                                          strides=(frame_stride, pitch, 1))
    roi[...] = np.ascontiguousarray(c.frames).view(np.uint8).reshape(n, h, rb)
    return buf


def _stage(gpu, c, name, levels, batch, **kw):
    store = [c.acq[i] for i in c.order] if c.order else c.acq
    f0 = store[0][2]
    for d in store[1:-2]:
        f0 *= d[1]
    n = len(c.frames)
    st = gpu.Stage(c.acq, c.dtype, c.method, storage_order=c.order, max_batch_frames=batch,
                   layer_slots=-(-n // f0) + 2, **kw)
    assert st.n_levels() == levels == len(c.ldims)
    assert st.dominant_kernel() == name
    return st


def _compare(st, c, what):
    st.finalize()
    for l in range(len(c.ldims)):
        assert st.frames_written(l) == c.fw[l], (what, l)
    for (l, layer), (buf, flags) in sorted(c.exp.items()):
        got, gflags = st.copy_layer(l, layer)
        assert_same_pixels(got, buf, c.dtype, f"{what} L{l} layer{layer}")
        assert (gflags == flags).all(), f"{what} has_data L{l} layer{layer}"


def _run_device(gpu, c, name, levels, pitch, frame_stride, off0, expect, batch, chunks=None):
    """Append c's frames from a poisoned, tightly sized device canvas and
    compare every layer and flag; expect = (direct, packed) frames."""
    import torch
    what = (f"{name} {DTYPE_NAMES[c.dtype]} {METHOD_NAMES[c.method]} pitch={pitch} "
            f"fs={frame_stride} off={off0}")
    n = len(c.frames)
    st = _stage(gpu, c, name, levels, batch)
    t = torch.from_numpy(_canvas(c, pitch, frame_stride, off0)).cuda()
    torch.cuda.synchronize()
    base = t.data_ptr()
    assert base % 16 == 0
    i = 0
    for k in chunks or [n]:
        st.append_strided(base + off0 + i * frame_stride, k, pitch, frame_stride, gpu.MEM_DEVICE)
        i += k
    assert i == n
    st.synchronize()  # the source is read asynchronously: before t goes
    assert st.frames_consumed() == n
    assert st.source_report() == expect, what
    assert st.dominant_kernel() == name
    del t
    _compare(st, c, what)
    st.close()


# ---------------------------------------------------------------------------
# 1, 2: the 2-D fused kernels read the pitched rows in place
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,method", [(U8, MEAN), (U16, MEAN), (F32, MEAN), (F64, MEAN),
                                          (I16, MIN)],
                         ids=["u8", "u16", "f32", "f64", "i16-min"])
def test_2d_direct_roi_of_a_canvas(gpu, dtype, method):
    """203 rows x 1072 bytes at row 3, byte column 32 of a 208-row canvas of
    1120-byte lines: interior, right-edge and bottom-edge regions."""
    c = _shallow2d(dtype, method)
    _run_device(gpu, c, _name2d(dtype, 0), 3, 1120, 208 * 1120, 3 * 1120 + 32, (3, 0), batch=2)


@pytest.mark.parametrize("dtype,method", [(U16, MEAN), (I8, MIN)], ids=["u16", "i8-min"])
def test_deep_2d_direct(gpu, dtype, method):
    """5 levels: the strip kernel's register levels 3-4 and the bottom / right
    edge replication under a pitch of W * bpp + 32."""
    c = _deep2d(dtype, method)
    pitch = 560 * BPP[dtype] + 32
    _run_device(gpu, c, _name2d(dtype, 0), 5, pitch, 523 * pitch, 0, (2, 0), batch=2)


@lru_cache(maxsize=1)
def _ragged2d():
    # u16 rows of 1062 bytes (no multiple of 16): two 512-byte interior regions
    # + 38 ragged bytes whose last 16-byte vector is partial; 203 -> 102 -> 51
    store = [(TIME, 0, 2, 1), (SPACE, 203, 64, 1), (SPACE, 531, 64, 1)]
    frames = _inputs(U16, 3, 203, 531, 6001)
    frames[2, 64:192] = 0
    return _case(store, U16, MEAN, frames)


def test_2d_direct_rows_no_multiple_of_16_bytes(gpu):
    """The pitch, not the row length, aligns the row starts: a 1062-byte ROI row
    still runs the interior kernel on its interior, and the partial last vector
    of a row -- the last one ends the allocation -- is read pixel by pixel.  The
    frame stride is no multiple of the pitch."""
    c = _ragged2d()
    _run_device(gpu, c, _name2d(U16, 0), 3, 1120, 203 * 1120 + 48, 16, (3, 0), batch=2)


# ---------------------------------------------------------------------------
# 3: the packed route, every unit of pack_frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U8, U16, F32, F64], ids=_ids)
def test_packed_every_unit(gpu, dtype):
    """Pitch 1072 + bpp at base + bpp: units of 1, 2, 4 and 8 bytes."""
    b = BPP[dtype]
    c = _shallow2d(dtype, MEAN)
    pitch = 1072 + b
    _run_device(gpu, c, _name2d(dtype, 0), 3, pitch, 205 * pitch, b, (0, 3), batch=2)


# ---------------------------------------------------------------------------
# 4: 2x2x2 -- whole z groups in place, the rest packed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [U16, F32], ids=_ids)
@pytest.mark.parametrize("chunks,expect", [([8, 8], (16, 0)), ([8, 3, 5], (8, 8))],
                         ids=["groups", "ragged"])
def test_2x2x2_direct_and_packed(gpu, dtype, chunks, expect):
    c = _vol(dtype, MEAN, 2)
    _run_device(gpu, c, KERNELS_3D["strip3d_pair"][1], 3, 1040, 256 * 1040, 0, expect, batch=8,
                chunks=chunks)


def test_2x2x2_wide_type_packs_everything(gpu):
    c = _vol(F64, MEAN, 2)
    _run_device(gpu, c, "level_kernel", 3, 1040, 256 * 1040, 0, (0, 16), batch=8,
                chunks=[8, 3, 5])


# ---------------------------------------------------------------------------
# 5: XY-swapped storage orders are packed (16-byte units), acquisition rows pitched
# ---------------------------------------------------------------------------
def test_xy_2d_packed(gpu):
    c = _xy2d(U16, MEAN)  # acquisition rows of 208 px = 416 bytes
    _run_device(gpu, c, XY_KERNELS["fused"][1], 3, 448, 536 * 448 + 64, 32, (0, 3), batch=2)


def test_xy_2x2x2_packed(gpu):
    c = _xyvol(U16, MEAN)  # acquisition rows of 256 px = 512 bytes
    _run_device(gpu, c, XY_KERNELS_3D["default"][1], 3, 544, 512 * 544, 0, (0, 16), batch=16,
                chunks=[8, 8])


# ---------------------------------------------------------------------------
# 6: host sources run no new kernel
# ---------------------------------------------------------------------------
def test_host_pageable_numpy_view(gpu):
    c = _shallow2d(U16, MEAN)
    n, h, w = c.frames.shape
    canvas = np.full((n, h + 5, w + 24), 0xFFFF, dtype=np.uint16)
    view = canvas[:, 3:3 + h, 16:16 + w]
    view[...] = c.frames
    assert not view.flags.c_contiguous
    st = _stage(gpu, c, _name2d(U16, 0), 3, 2)
    st.append(view)
    assert st.frames_consumed() == n  # copied into staging before append returned
    canvas[...] = 0xFFFF
    st.synchronize()
    assert st.source_report() == (0, 0)
    _compare(st, c, "pageable view")
    st.close()


@pytest.mark.parametrize("canvas_rows", [203, 208], ids=["one-copy", "copy-per-frame"])
def test_host_pinned_canvas(gpu, canvas_rows):
    """frame_stride == H * row_stride takes one 2-D copy per batch, any other
    one per frame."""
    c = _shallow2d(U16, MEAN)
    n = len(c.frames)
    pitch, fs, off0 = 1120, canvas_rows * 1120, 32
    host = _canvas(c, pitch, fs, off0)
    hb = gpu.HostBuffer(host.size)
    hb.array[:] = host
    st = _stage(gpu, c, _name2d(U16, 0), 3, 2)
    st.append_strided(hb.ptr + off0, n, pitch, fs, gpu.MEM_HOST_PINNED)
    st.synchronize()
    assert st.frames_consumed() == n
    assert st.source_report() == (0, 0)
    _compare(st, c, f"pinned canvas rows={canvas_rows}")
    st.close()
    hb.close()


def test_host_pinned_buffer_object(gpu):
    """Stage.append_strided(HostBuffer, ...) appends from the buffer's start."""
    c = _shallow2d(U16, MEAN)
    n = len(c.frames)
    host = _canvas(c, 1104, 203 * 1104, 0)
    hb = gpu.HostBuffer(host.size)
    hb.array[:] = host
    st = _stage(gpu, c, _name2d(U16, 0), 3, 2)
    st.append_strided(hb, n, 1104, 203 * 1104)
    st.synchronize()
    assert st.source_report() == (0, 0)
    _compare(st, c, "pinned HostBuffer")
    st.close()
    hb.close()


# ---------------------------------------------------------------------------
# 7: contiguous strides are aqz_stage_append
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["shallow2d", "vol"])
def test_contiguous_strides_are_append(gpu, geom):
    if geom == "shallow2d":
        c, name, batch, pitch = _shallow2d(U16, MEAN), _name2d(U16, 0), 2, 1072
    else:
        c, name, batch, pitch = _vol(U16, MEAN, 2), KERNELS_3D["strip3d_pair"][1], 8, 1024
    h = c.frames.shape[1]
    _run_device(gpu, c, name, 3, pitch, h * pitch, 0, (0, 0), batch=batch)


# ---------------------------------------------------------------------------
# 8: refusals
# ---------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu):
    import torch
    c = _shallow2d(U16, MEAN)
    n, h, w = c.frames.shape
    rb, pitch = 2 * w, 1120
    fs = 208 * pitch
    t = torch.from_numpy(_canvas(c, pitch, fs, 0)).cuda()
    torch.cuda.synchronize()
    base = t.data_ptr()
    st = _stage(gpu, c, _name2d(U16, 0), 3, 2)
    bad = [
        ("row_stride < W*bpp", base, n, rb - 2, fs),
        ("frame_stride short", base, n, pitch, (h - 1) * pitch + rb - 2),
        ("row_stride % bpp", base, n, pitch + 1, fs),
        ("frame_stride % bpp", base, n, pitch, fs + 1),
        ("address % bpp", base + 1, n, pitch, fs),
        ("n_frames * frame_stride overflows", base, n, pitch, 1 << 63),
    ]
    for why, ptr, k, rs, fst in bad:
        with pytest.raises(gpu.AqzError) as e:
            st.append_strided(ptr, k, rs, fst, gpu.MEM_DEVICE)
        assert e.value.status == 1, why
        assert "append_strided" in str(e.value), why
        assert [st.frames_written(l) for l in range(3)] == [0, 0, 0], why
        assert st.source_report() == (0, 0), why
    for mem in (gpu.MEM_HOST, gpu.MEM_HOST_PINNED):  # refused before any host byte is read
        with pytest.raises(gpu.AqzError) as e:
            st.append_strided(base, n, rb - 2, fs, mem)
        assert e.value.status == 1
    # the stage is not in a sticky state: a valid append matches the oracle
    st.append_strided(base, n, pitch, fs, gpu.MEM_DEVICE)
    st.synchronize()
    assert st.source_report() == (3, 0)
    del t
    _compare(st, c, "after refusals")
    st.close()


def test_level0_split_on_host_stage_refuses(gpu):
    c = _shallow2d(U16, MEAN)
    n = len(c.frames)
    host = _canvas(c, 1120, 203 * 1120, 0)
    st = gpu.Stage(c.acq, c.dtype, c.method, max_batch_frames=2, layer_slots=4,
                   level0_split_on_host=True)
    with pytest.raises(gpu.AqzError) as e:
        st.append_strided(host.ctypes.data, n, 1120, 203 * 1120, gpu.MEM_HOST)
    assert e.value.status == 1 and "level0_split_on_host" in str(e.value)
    assert st.frames_written(0) == 0
    st.close()


# ---------------------------------------------------------------------------
# 9: the Python mirror passes a view's strides on
# ---------------------------------------------------------------------------
def test_python_append_of_a_cuda_view(gpu):
    import torch
    c = _shallow2d(U16, MEAN)
    n, h, w = c.frames.shape
    # uint16 bit patterns as int16 (torch has no uint16 arithmetic; none is needed)
    canvas = torch.full((n, h + 5, w + 24), -1, dtype=torch.int16, device="cuda")
    view = canvas[:, 2:2 + h, 8:8 + w]
    view.copy_(torch.from_numpy(c.frames.view(np.int16)))
    assert not view.is_contiguous()
    layers = []
    for src in (view, view.contiguous()):
        st = _stage(gpu, c, _name2d(U16, 0), 3, 2)
        st.append(src)
        st.synchronize()
        layers.append(st.source_report())
        _compare(st, c, "cuda view" if src is view else "contiguous copy")
        st.close()
    assert layers == [(3, 0), (0, 0)]  # 16-byte column and pitch: read in place
    st = _stage(gpu, c, _name2d(U16, 0), 3, 2)
    with pytest.raises(AssertionError):
        st.append(canvas[:, :h, ::2][:, :, :w // 2])  # last stride of two elements
    with pytest.raises(AssertionError):
        st.append(np.zeros((n, h, 2 * w), np.uint16)[:, :, ::2])
    st.close()
