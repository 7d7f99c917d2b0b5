"""Every pyramid kernel x dtype x method on interior regions, vs the CPU oracle.

The kernels of aqz_kernels.hip are templates over 10 dtypes x 4 methods, and
the fast (interior) paths -- packing, wave shuffles, the LDS cascade, the XY
load -- were run by the older tests for part of that matrix only.  Each case
here first creates its stage and asserts n_levels() and dominant_kernel(),
then runs it and compares every chunk layer and every has_data flag with the
oracle (tests/helpers.py: bit-exact integers, floats bit-exact off NaN with
NaN positions equal).  Chunks are 64 x 64 px everywhere, so regions are 64
rows (rh_log2 == 6) x 512 bytes; every geometry has interior regions plus
ragged right and bottom edge regions where it can.  Inputs: synthetic_frames
(full-range integers), floats with a seeded half of the pixels negated, then
with_specials (integer min/max; NaN, +-0, +-inf, denormals, +-max).  The
deep geometry's second frame is _blocky() instead: with specials in a fifth
of the pixels, MIN / MAX of the 64 or 256 pixels under a level-3 or level-4
pixel is nearly always the dtype's extreme, and a first defect build of
group 2 (below) passed for that reason.

What each group runs that no earlier test ran (T = pixel type, M = method):

1. 2-D shallow (1072-byte rows x 203, 3 levels): fused_pyramid_strip<T, M>
   for T = i8, i32 with M = DECIMATE, MIN, MAX; fused_pyramid<T, M> (knob
   128) for T = i8, i32 with every M; fused_pyramid<T, M> for T = u64, i64,
   f64 with every M on 64-row regions (levels 1-2: the shfl_xor_t /
   shfl_down_t 8-byte path).
2. 2-D deep (560 x 523 px, 5 levels, odd 33 x 35 last level): the strip
   kernel's register levels 3-4 for T = i8, i32 (every M) and for u8, u32,
   f32 with DECIMATE / MAX; lean_pair<T, M, 3> (LDS levels 3-4 of
   fused_pyramid) for the 8-byte types with every M and, under knob 128, for
   the seven narrow types.
3. 2x2x2 (z = 8, 1024-byte rows x 256; z chunk 2: G = 4, z chunk 4: G = 2):
   fused_pyramid_strip3d_pair (three variants), fused_pyramid_strip3d (two)
   and fused_pyramid_3d for T = i8, i32 with every M; the G = 2 schedule
   (z halves at level 1 only) for every narrow T.  u64 / i64 / f64 report
   level_kernel.
4. XY-swapped 2-D: fused_pyramid_strip<T, M, XY> for T = i8, i32 (every M)
   and for the other narrow types with DECIMATE / MAX; transpose_frames +
   fused_pyramid_strip for T = i8, i32 and M != MEAN; transpose_frames<u64>
   + fused_pyramid for the 8-byte types on 64-row regions.
5. XY-swapped 2x2x2: fused_pyramid_strip3d<.., XY> and
   fused_pyramid_strip3d_pair<.., XY> for T = i8, i32 and, for every narrow
   T, with MIN.
6. A device-resident source at every pixel-aligned offset of a 16-byte
   line: the unaligned fallbacks of fused_params / run_batch (whole frame
   through fused_pyramid_edge's scalar loads, 2x2x2 through level_kernel's
   fetch, XY through transpose_frames), which no test and no benchmark had
   run.  Read before the first run: every 16-byte load of those paths is
   behind vec_rows (generic_region), fast_ok (the interior kernels), the
   `% 16` test of `idle` (2x2x2) or of `direct` (load_region_xy); fetch and
   transpose_frames load single pixels.  No unguarded wide load was found.

Geometry notes (where the issue's figures and the engine's answers needed
matching): the 8-byte types' 2x2x2 dims give 3 levels with z chunk 2 (level
2 keeps Y = 128) and 2 levels with z chunk 4; both are asserted against the
oracle's level list.

Defect builds (scratch copies, never committed; each changes values only).
"old" = test_gpu_parity.py + test_gpu_golden.py of the parent commit:

| group | defect                                                        | old    | new group |
|-------|---------------------------------------------------------------|--------|-----------|
| 1 | fast_pass level 2 of fused_pyramid: i32 MIN compared as u32       | passes | fails: [i32-knob128] |
| 2 | strip kernel level 4: i8 MIN compared as u8                       | passes | fails: [i8-default] |
| 3 | launch_fused_pyramid_3d: the i8 row dispatched to u8              | passes | fails: all six [i8-*] |
| 4 | launch_interior, XY branch: i32 run as u32                        | passes | fails: [i32-fused] |
| 5 | XY single-plane 2x2x2 launch: MIN instantiated as MAX             | passes | fails: 14 cases (default, single) |

Every failure above is an assert_same_pixels mismatch; all 239 old tests
pass on each defect build.  Defect 2 was first run against a deep geometry
of two synthetic_frames + with_specials frames and was missed (every level-4
MIN was the i8 minimum either way); the blocky frame was added for it.

Group 6 has no defect build: breaking an alignment guard would issue
misaligned vector loads.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest

from helpers import assert_same_pixels, expected_stage_layers, with_specials
from oracle_bindings import (DECIMATE, DTYPE_NAMES, F32, F64, I8, I16, I32, I64,
                             MAX, MEAN, METHOD_NAMES, MIN, NP_DTYPES, SPACE, TIME,
                             U8, U16, U32, U64, synthetic_frames)
from test_gpu_parity import KERNELS_3D, XY_KERNELS, XY_KERNELS_3D

pytestmark = pytest.mark.gpu

ALL_DTYPES = [U8, U16, U32, U64, I8, I16, I32, I64, F32, F64]
NARROW = [U8, U16, U32, I8, I16, I32, F32]  # launch_fused_pyramid_3d's rows
WIDE = [U64, I64, F64]
ALL_METHODS = [DECIMATE, MEAN, MIN, MAX]
BPP = {k: np.dtype(v).itemsize for k, v in NP_DTYPES.items()}
_ids = lambda d: DTYPE_NAMES[d]  # noqa: E731

# storage-order dims, acquisition-order dims (None: the same), storage order,
# input frames in acquisition order, and the oracle's layers for them
Case = namedtuple("Case", "acq order dtype method frames exp fw ldims")


def _inputs(dtype, n, h, w, seed):
    fr = synthetic_frames(dtype, n, h, w, seed)
    if dtype in (F32, F64):
        # synthetic_frames makes no negative ordinary floats
        neg = np.random.default_rng(seed + 3).random(fr.shape) < 0.5
        fr[neg] = -fr[neg]
    return with_specials(fr, dtype, seed + 7)


def _blocky(dtype, h, w, seed):
    """One frame of 4 x 4 px blocks, each a full-range random value (floats:
    random sign) with a little per-pixel jitter and no specials.  With 20 %
    specials in every frame the MIN / MAX of 64 or 256 pixels is almost always
    the dtype's extreme, whatever the kernel does with the rest; here a
    level-3 or level-4 pixel reduces 4 or 16 unrelated values of mixed sign,
    so the deep levels keep full-range variation."""
    bh, bw = -(-h // 4), -(-w // 4)
    base = synthetic_frames(dtype, 1, bh, bw, seed)[0]
    jit = synthetic_frames(dtype, 1, h, w, seed + 1)[0]
    if dtype in (F32, F64):
        neg = np.random.default_rng(seed + 3).random(base.shape) < 0.5
        base[neg] = -base[neg]
    big = np.repeat(np.repeat(base, 4, axis=0), 4, axis=1)[:h, :w]
    if dtype in (F32, F64):
        return big + jit / NP_DTYPES[dtype](65536)
    return big ^ (jit & NP_DTYPES[dtype](3))


def _case(store, dtype, method, frames, xy=False):
    """Oracle layers of `frames` (acquisition order) for storage dims `store`."""
    n = len(store)
    if xy:
        acq = store[:-2] + [store[-1], store[-2]]
        order = list(range(n - 2)) + [n - 1, n - 2]
        stored = np.ascontiguousarray(frames.transpose(0, 2, 1))
    else:
        acq, order, stored = store, None, frames
    exp, fw, ldims = expected_stage_layers(store, dtype, method, stored)
    return Case(acq, order, dtype, method, frames, exp, fw, ldims)


def _run(gpu, c, name, levels, knobs=0, batch=0, chunks=None, dev_off=None):
    """Create the stage, assert the kernel it will run, run it, compare every
    layer and flag.  dev_off: append from a device tensor at base + dev_off."""
    store = [c.acq[i] for i in c.order] if c.order else c.acq
    f0 = store[0][2]
    for d in store[1:-2]:
        f0 *= d[1]
    n = len(c.frames)
    kw = {"knobs": knobs} if knobs else {}
    st = gpu.Stage(c.acq, c.dtype, c.method, storage_order=c.order,
                   max_batch_frames=batch, layer_slots=-(-n // f0) + 2, **kw)
    what = f"{name} {DTYPE_NAMES[c.dtype]} {METHOD_NAMES[c.method]} off={dev_off}"
    assert st.n_levels() == levels == len(c.ldims), what
    assert st.dominant_kernel() == name, what
    for l in range(levels):
        assert [tuple(x) for x in st.level_dims(l)] == [tuple(x) for x in c.ldims[l]]
    chunks = chunks or [n]
    assert sum(chunks) == n
    if dev_off is None:
        i = 0
        for k in chunks:
            st.append(np.ascontiguousarray(c.frames[i:i + k]))
            i += k
    else:
        import torch
        raw = np.ascontiguousarray(c.frames).view(np.uint8).reshape(-1)
        fbytes = raw.size // n
        t = torch.empty(raw.size + 64, dtype=torch.uint8, device="cuda")
        base = t.data_ptr()
        assert base % 16 == 0 and dev_off % BPP[c.dtype] == 0 and dev_off <= 64
        t[dev_off:dev_off + raw.size].copy_(torch.from_numpy(raw))
        torch.cuda.synchronize()
        i = 0
        for k in chunks:
            st.append_ptr(base + dev_off + i * fbytes, k)
            i += k
        st.synchronize()  # the source is read asynchronously: before t goes
        del t
    st.finalize()
    for l in range(levels):
        assert st.frames_written(l) == c.fw[l], (what, l)
    for (l, layer), (buf, flags) in sorted(c.exp.items()):
        got, gflags = st.copy_layer(l, layer)
        assert_same_pixels(got, buf, c.dtype, f"{what} L{l} layer{layer}")
        assert (gflags == flags).all(), f"{what} has_data L{l} layer{layer}"
    st.close()


# ---------------------------------------------------------------------------
# geometries (each oracle result is computed once and shared by the cases of
# one dtype, which pytest runs back to back)
# ---------------------------------------------------------------------------
@lru_cache(maxsize=4)
def _shallow2d(dtype, method):
    # 1072-byte rows: two 512-byte regions + 48 ragged bytes; 203 -> 102 -> 51
    w = 1072 // BPP[dtype]
    store = [(TIME, 0, 2, 1), (SPACE, 203, 64, 1), (SPACE, w, 64, 1)]
    frames = _inputs(dtype, 3, 203, w, 1000 + dtype)
    frames[2, 64:192] = 0  # chunk rows without data in the partial last layer
    return _case(store, dtype, method, frames)


@lru_cache(maxsize=4)
def _deep2d(dtype, method):
    # 560 -> 280 -> 140 -> 70 -> 35 and 523 -> 262 -> 131 -> 66 -> 33
    store = [(TIME, 0, 1, 1), (SPACE, 523, 64, 1), (SPACE, 560, 64, 1)]
    frames = _inputs(dtype, 2, 523, 560, 2000 + dtype)
    frames[1] = _blocky(dtype, 523, 560, 2100 + dtype)
    frames[1, 128:384] = 0
    return _case(store, dtype, method, frames)


@lru_cache(maxsize=8)
def _vol(dtype, method, zchunk):
    # two stacks of 8 planes, 1024-byte rows x 256
    w = 1024 // BPP[dtype]
    store = [(TIME, 0, 1, 1), (SPACE, 8, zchunk, 1), (SPACE, 256, 64, 1), (SPACE, w, 64, 1)]
    return _case(store, dtype, method, _inputs(dtype, 16, 256, w, 3000 + dtype + zchunk))


@lru_cache(maxsize=4)
def _xy2d(dtype, method):
    # acquisition (Y, X) = (1072 / bpp, 208): storage 208 rows x 1072 / bpp
    # columns; 208 rows (not 203) keep the acquisition rows 16-byte multiples
    w = 1072 // BPP[dtype]
    store = [(TIME, 0, 2, 1), (SPACE, 208, 64, 1), (SPACE, w, 64, 1)]
    return _case(store, dtype, method, _inputs(dtype, 3, w, 208, 4000 + dtype), xy=True)


@lru_cache(maxsize=4)
def _xyvol(dtype, method):
    # acquisition (z, y, x) = (8, 1024 / bpp, 256), z chunk 2
    w = 1024 // BPP[dtype]
    store = [(TIME, 0, 1, 1), (SPACE, 8, 2, 1), (SPACE, 256, 64, 1), (SPACE, w, 64, 1)]
    return _case(store, dtype, method, _inputs(dtype, 16, w, 256, 5000 + dtype), xy=True)


def _name2d(dtype, knobs):
    return "fused_pyramid_strip" if BPP[dtype] <= 4 and not knobs & 128 else "fused_pyramid"


# ---------------------------------------------------------------------------
# 1, 2: 2-D interior regions, every dtype and method
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [0, 128], ids=["default", "knob128"])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=_ids)
def test_shallow_2d_every_dtype_method(gpu, knobs, dtype):
    """Group 1: 3 levels, 3 frames in batches of 2 (a partial last layer)."""
    for m in ALL_METHODS:
        _run(gpu, _shallow2d(dtype, m), _name2d(dtype, knobs), 3, knobs=knobs, batch=2)


@pytest.mark.parametrize("knobs", [0, 128], ids=["default", "knob128"])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=_ids)
def test_deep_2d_every_dtype_method(gpu, knobs, dtype):
    """Group 2: 5 levels -- the strip kernel's register levels 3-4, and
    fused_pyramid's LDS-cascaded levels 3-4 (8-byte types; knob 128: all)."""
    for m in ALL_METHODS:
        _run(gpu, _deep2d(dtype, m), _name2d(dtype, knobs), 5, knobs=knobs, batch=2)


# ---------------------------------------------------------------------------
# 3: 2x2x2, every kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS_3D))
@pytest.mark.parametrize("dtype", NARROW, ids=_ids)
def test_2x2x2_every_kernel_dtype_method(gpu, kernel, dtype):
    """Group 3: z chunk 2 (G = 4) and z chunk 4 (z halves at level 1 only,
    G = 2); appends of [8, 3, 5] leave and regain group alignment."""
    knobs, name = KERNELS_3D[kernel]
    for zchunk in (2, 4):
        for m in ALL_METHODS:
            c = _vol(dtype, m, zchunk)
            assert [l[1][1] for l in c.ldims] == ([8, 4, 2] if zchunk == 2 else [8, 4, 4])
            _run(gpu, c, name, 3, knobs=knobs, batch=8, chunks=[8, 3, 5])


@pytest.mark.parametrize("dtype", WIDE, ids=_ids)
def test_2x2x2_wide_types_take_level_kernel(gpu, dtype):
    """8-byte pixels have no fused 2x2x2 kernel: the same dims (128 px rows)
    must report level_kernel and still be oracle-exact."""
    for zchunk, levels in ((2, 3), (4, 2)):
        for m in ALL_METHODS:
            _run(gpu, _vol(dtype, m, zchunk), "level_kernel", levels, batch=8,
                 chunks=[8, 3, 5])


# ---------------------------------------------------------------------------
# 4, 5: XY-swapped storage order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(XY_KERNELS))
@pytest.mark.parametrize("dtype", NARROW, ids=_ids)
def test_xy_2d_every_dtype_method(gpu, path, dtype):
    """Group 4: the strip kernel's XY load, and (knob 4096) the separate
    transpose pass, 3 levels, 3 frames in batches of 2."""
    knobs, name = XY_KERNELS[path]
    for m in ALL_METHODS:
        _run(gpu, _xy2d(dtype, m), name, 3, knobs=knobs, batch=2)


@pytest.mark.parametrize("dtype", WIDE, ids=_ids)
def test_xy_2d_wide_types_transpose_pass(gpu, dtype):
    for m in (MEAN, MAX):
        _run(gpu, _xy2d(dtype, m), "transpose_frames + fused_pyramid", 3, batch=2)


@pytest.mark.parametrize("path", sorted(XY_KERNELS_3D))
@pytest.mark.parametrize("dtype", NARROW, ids=_ids)
def test_xy_2x2x2_every_kernel_dtype(gpu, path, dtype):
    """Group 5: whole z groups ([8, 8]) take the XY load; [6, 10] also needs
    the generic cascade and is transposed first."""
    knobs, name = XY_KERNELS_3D[path]
    for m in (MEAN, MIN):
        for chunks in ([8, 8], [6, 10]):
            _run(gpu, _xyvol(dtype, m), name, 3, knobs=knobs, batch=16, chunks=chunks)


# ---------------------------------------------------------------------------
# 6: device-resident source at every pixel-aligned offset of a 16-byte line
# ---------------------------------------------------------------------------
def _offsets(dtype):
    b = BPP[dtype]
    return sorted({b, 8, 16 - b, 16})  # 16: the aligned control


@pytest.mark.parametrize("geom", ["shallow2d", "vol", "xy2d", "xyvol"])
@pytest.mark.parametrize("dtype", [U8, U16, F32, F64], ids=_ids)
def test_device_source_at_every_alignment(gpu, geom, dtype):
    """aqz_stage_append accepts any pixel-aligned device address: only a
    16-byte-aligned one takes the fast kernels, the others the scalar-load
    fallbacks, and every layer and has_data flag equals the oracle's at
    every offset."""
    wide = BPP[dtype] == 8
    if geom == "shallow2d":
        c, name, kw = _shallow2d(dtype, MEAN), _name2d(dtype, 0), dict(batch=2)
    elif geom == "vol":
        c = _vol(dtype, MEAN, 2)
        name = "level_kernel" if wide else KERNELS_3D["strip3d_pair"][1]
        kw = dict(batch=8, chunks=[8, 3, 5])
    elif geom == "xy2d":
        c = _xy2d(dtype, MEAN)
        name = "transpose_frames + fused_pyramid" if wide else XY_KERNELS["fused"][1]
        kw = dict(batch=2)
    else:
        c = _xyvol(dtype, MEAN)
        name = "level_kernel" if wide else XY_KERNELS_3D["default"][1]
        kw = dict(batch=16, chunks=[6, 10])
    for off in _offsets(dtype):
        _run(gpu, c, name, 3, dev_off=off, **kw)
