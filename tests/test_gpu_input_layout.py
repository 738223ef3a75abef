"""Extraction from padded, offset and device-resident input.

Every other GPU test hands sgpu_extract* a dense host array (rows w apart, in the library's own
aligned upload buffer), so each ingest kernel only ever sees "everything vectorises" (w % 4 == 0)
or "nothing does".  Here the caller's buffer has rows `stride` apart with poisoned padding
(input_layouts.py: u8 0 / 255, f32 NaN), starts at odd byte offsets inside a device allocation
(devmem.py), and comes in as host, staged and device input, u8, f32 and colour.  The expected
values are the CPU oracle's on the dense images: levels 0 and 1 of octave 0 and every keypoint bit
for bit, descriptors within DESC_L2_TOL (bit for bit from the exact kernel), whatever the layout.

Which ingest ran is read from pyramid_plan(): the kind of the launch that holds level (0, 0).  The
expectations are the launchers' predicates (gauss_dispatch, gauss_tile_supported,
gauss_duo_supported) applied to the layout:
  aligned  (row and image stride % 4 == 0, base % 16 == 0): tiles where tiles are forced, the tile
           duo / paired launch holding (0, 0) and (0, 1) where those are forced (u8; f32 input has
           a compiled tile duo but no paired-level kernel for its first level);
  quad     (u8, as aligned but base % 16 == 4): the same under the tile and paired forms (their
           loads are 4-byte quads); k_gauss_lean wants 16 bytes, so the wave forms run scalar --
           still a `level` launch;
  scalar   (a stride % 4 != 0, or a base the element type's quad does not divide): one `level`
           launch for (0, 0) in every form.
With the workgroup-strip kernel (GAUSS_BLOCK) and with tiles off, (0, 0) is a `level` launch for
every layout: the planner pairs levels only when forced or from 128 MB.

Not run here: colour input has no level comparison (the oracle's level dump takes u8 only; its keys
and descriptors are compared), and the first-octave resampling and extract_stream cases run the
shipped form only (they replace or bypass the first level's caller-side read)."""
import numpy as np
import pytest

import devmem
import input_layouts as IL
import oracle_py as O
import sgpu
from sgpu_types import default_options

pytestmark = pytest.mark.gpu

DESC_L2_TOL = 1e-4   # test_gpu_parity.py: BASELINE.json north_star, descriptor L2 < 1e-4

C = sgpu.SiftContext
# (name, debug flags, pairs, strips)
FORMS = [
    ("shipped", 0, C.PAIRS_END, C.STRIPS_RULE),
    ("block", C.DEBUG_GAUSS_BLOCK, C.PAIRS_END, C.STRIPS_RULE),
    ("tiles_off", C.DEBUG_GAUSS_TILE_OFF, C.PAIRS_END, C.STRIPS_RULE),
    ("tiles_always", C.DEBUG_GAUSS_TILE_ALWAYS, C.PAIRS_END, C.STRIPS_RULE),
    ("duo", C.DEBUG_DUO_ALWAYS, C.PAIRS_END, C.STRIPS_RULE),
    ("tile_duo", C.DEBUG_GAUSS_TILE_ALWAYS | C.DEBUG_DUO_ALWAYS, C.PAIRS_END, C.STRIPS_RULE),
]
FORM_COOP = ("duo_coop", C.DEBUG_DUO_ALWAYS, C.PAIRS_END, C.STRIPS_COOP)   # shape B only
MULTI_LEVEL = {"duo", "trio", "tile_duo", "tile_duo_one"}

_REF = {}   # (images key, option key) -> per image (keys, descriptors), levels (0, 0) / (0, 1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _opt_key(opts):
    return (opts.octave_min, opts.preprocess_on_cpu)


def _reference(key, dense_u8, opts, gray_f32=None):
    """The oracle's features of every image and levels (0, 0), (0, 1) of the first and the last,
    once per image set and option set.  gray_f32: float images for the oracle instead (no levels:
    the oracle's level dump takes u8)."""
    k = (key, _opt_key(opts))
    if k not in _REF:
        if gray_f32 is None:
            feats = [O.extract(im, opts) for im in dense_u8]
            last = len(dense_u8) - 1
            levels = {i: [O.gaussian(dense_u8[i], 0, lvl, opts) for lvl in (0, 1)]
                      for i in {0, last}}
        else:
            feats = [O.extract_f32(im, opts) for im in gray_f32]
            levels = None
        for kk, dd in feats:
            kk.setflags(write=False)
            dd.setflags(write=False)
        _REF[k] = (feats, levels)
    return _REF[k]


def _layout_class(elem_bytes, stride, h, base):
    """aligned / quad / scalar, from the predicates (strides in elements, base in bytes)."""
    quad = 4 * elem_bytes   # bytes of a four-element load: 4 (u8) or 16 (f32)
    if stride % 4 or (stride * h) % 4 or base % quad:
        return "scalar"
    return "aligned" if base % 16 == 0 else "quad"


def _check_plan(plan, form, cls, u8, what):
    """The launch holding level (0, 0) is of the kind the layout's class allows under the form."""
    entry = [(k, lv) for k, lv in plan if (0, 0) in lv]
    assert len(entry) == 1, (what, plan)
    kind, levels = entry[0]
    vector_tiles = cls in ("aligned", "quad")
    if form in ("block", "tiles_off") or not vector_tiles:
        assert kind == "level" and levels == [(0, 0)], (what, form, cls, plan)
    elif form == "tiles_always":
        assert kind in ("tile", "tile_two"), (what, form, cls, plan)
    elif form == "tile_duo":
        assert kind in ("tile_duo", "tile_duo_one") and levels[:2] == [(0, 0), (0, 1)], (what, form, cls, plan)
    elif form in ("duo", "duo_coop"):
        if u8:
            assert kind == "duo" and levels == [(0, 0), (0, 1)], (what, form, cls, plan)
        else:
            assert kind not in MULTI_LEVEL and levels == [(0, 0)], (what, form, cls, plan)


def _check_features(ctx, feats, what, exact):
    assert ctx.total() == sum(len(k) for k, _ in feats), what
    for i, (rk, rd) in enumerate(feats):
        k, d = ctx.features(i)
        assert k.shape == rk.shape, f"{what} image {i}: {k.shape} features, oracle {rk.shape}"
        if not len(k):
            continue
        assert not np.isnan(k).any() and not np.isnan(d).any(), f"{what} image {i}: NaN leaked"
        diff = _bits(k) != _bits(rk)
        assert not diff.any(), f"{what} image {i}: key bits differ at rows {np.where(diff.any(1))[0][:8]}"
        if exact:
            assert np.array_equal(_bits(d), _bits(rd)), f"{what} image {i}: exact descriptor bits"
        else:
            l2 = np.linalg.norm(d.astype(np.float64) - rd.astype(np.float64), axis=1).max()
            assert l2 < DESC_L2_TOL, f"{what} image {i}: descriptor L2 {l2}"


def _check_levels(ctx, levels, what):
    for i, want in levels.items():
        for lvl in (0, 1):
            g = ctx.gaussian(i, 0, lvl)
            assert not np.isnan(g).any(), f"{what} image {i} level {lvl}: NaN leaked"
            assert np.array_equal(_bits(g), _bits(want[lvl])), f"{what} image {i} level (0, {lvl})"


def _run_forms(ctx, run, feats, levels, cls, u8, what, forms, opts=None):
    """run() under every form (and once under the exact descriptor kernel in the shipped form):
    levels, keys, descriptors, and the kind of launch that held level (0, 0)."""
    ctx.set_options(opts or default_options())
    try:
        for name, flags, pairs, strips in forms:
            ctx.set_schedule(C.TRIO_OFF, pairs)
            ctx.set_duo_strips(strips)
            ctx.set_debug_flags(flags)
            run()
            w = f"{what} [{name}]"
            if cls is not None:
                _check_plan(ctx.pyramid_plan(), name, cls, u8, w)
            if levels is not None:
                _check_levels(ctx, levels, w)
            _check_features(ctx, feats, w, exact=False)
        ctx.set_schedule()
        ctx.set_duo_strips(C.STRIPS_RULE)
        with ctx.exact_descriptors():
            run()
            _check_features(ctx, feats, f"{what} [exact]", exact=True)
    finally:
        ctx.set_schedule()
        ctx.set_duo_strips(C.STRIPS_RULE)
        ctx.set_debug_flags(0)
        ctx.set_options(default_options())


def _forms(shape):
    return FORMS + ([FORM_COOP] if shape == "B" else [])


def _id(layout):
    return "-".join(str(v) for v in layout)


HOST_U8 = [l for l in IL.U8_LAYOUTS if l[2] == 0]


@pytest.mark.parametrize("layout", HOST_U8, ids=_id)
def test_host_u8(gpu_ctx, layout):
    shape, stride, _ = layout
    n, w, h = IL.SHAPES[shape]
    dense = IL.images(shape)
    buf = IL.pad(dense, stride)
    feats, levels = _reference(shape, dense, default_options())
    _run_forms(gpu_ctx, lambda: gpu_ctx.extract(buf, shape=(n, h, w), stride=stride), feats, levels,
               _layout_class(1, stride, h, 0), True, f"host u8 {layout}", _forms(shape))


@pytest.mark.parametrize("layout", HOST_U8, ids=_id)
def test_staged_u8(gpu_ctx, layout):
    shape, stride, _ = layout
    n, w, h = IL.SHAPES[shape]
    dense = IL.images(shape)
    feats, levels = _reference(shape, dense, default_options())
    gpu_ctx.stage(IL.pad(dense, stride), stride=stride, shape=(n, h, w))
    _run_forms(gpu_ctx, gpu_ctx.extract_staged, feats, levels, _layout_class(1, stride, h, 0), True,
               f"staged u8 {layout}", _forms(shape))


@pytest.mark.parametrize("layout", IL.U8_LAYOUTS, ids=_id)
def test_device_u8(gpu_ctx, layout):
    shape, stride, offset = layout
    n, w, h = IL.SHAPES[shape]
    dense = IL.images(shape)
    feats, levels = _reference(shape, dense, default_options())
    with devmem.uploaded(IL.pad(dense, stride), offset) as ptr:
        assert (ptr - offset) % 256 == 0
        _run_forms(gpu_ctx,
                   lambda: gpu_ctx.extract(ptr, shape=(n, h, w, stride), device_ptr=True),
                   feats, levels, _layout_class(1, stride, h, ptr), True, f"device u8 {layout}",
                   _forms(shape))


def test_device_u8_split_batch(gpu_ctx):
    """Two parts of one device batch (2 + 1 images): part 1 starts 2 * 204 * 97 bytes in, 8 mod 16,
    so the parts differ in alignment.  (The split runs octave by octave on two streams; no plan
    expectation.)"""
    n, w, h = IL.SHAPES["A"]
    stride = 204
    assert (2 * stride * h) % 16 == 8
    dense = IL.images("A")
    feats, levels = _reference("A", dense, default_options())
    gpu_ctx.set_options(default_options())
    with devmem.uploaded(IL.pad(dense, stride)) as ptr:
        try:
            for flags, exact in ((C.DEBUG_PARTS2, False),
                                 (C.DEBUG_PARTS2 | C.DEBUG_EXACT_DESCRIPTOR, True)):
                gpu_ctx.set_debug_flags(flags)
                gpu_ctx.extract(ptr, shape=(n, h, w, stride), device_ptr=True)
                _check_levels(gpu_ctx, levels, "split batch")
                _check_features(gpu_ctx, feats, "split batch", exact)
        finally:
            gpu_ctx.set_debug_flags(0)


def _f32_images():
    return IL.images("A").astype(np.float32) / np.float32(255.0)


@pytest.mark.parametrize("stride", sorted({s for _, s, _ in IL.F32_LAYOUTS}))
def test_host_f32(gpu_ctx, stride):
    """Float input holding u8 / 255 gives the u8 path's bits (test_float_input_matches_u8), so the
    u8 oracle's values apply; the padding is NaN."""
    n, w, h = IL.SHAPES["A"]
    feats, levels = _reference("A", IL.images("A"), default_options())
    buf = IL.pad(_f32_images(), stride)
    _run_forms(gpu_ctx, lambda: gpu_ctx.extract(buf, shape=(n, h, w), stride=stride), feats, levels,
               _layout_class(4, stride, h, 0), False, f"host f32 stride {stride}", FORMS)


@pytest.mark.parametrize("layout", IL.F32_LAYOUTS, ids=_id)
def test_device_f32(gpu_ctx, layout):
    shape, stride, offset = layout
    n, w, h = IL.SHAPES[shape]
    feats, levels = _reference(shape, IL.images(shape), default_options())
    with devmem.uploaded(IL.pad(_f32_images(), stride), offset) as ptr:
        _run_forms(gpu_ctx,
                   lambda: gpu_ctx.extract(ptr, shape=(n, h, w, stride), device_ptr=True,
                                           dtype=np.float32),
                   feats, levels, _layout_class(4, stride, h, ptr), False, f"device f32 {layout}",
                   FORMS)


@pytest.mark.parametrize("offset", (None,) + IL.COLOR_OFFSETS, ids=lambda o: "host" if o is None else f"device+{o}")
@pytest.mark.parametrize("fmt,stride", IL.COLOR_LAYOUTS)
def test_color(gpu_ctx, fmt, stride, offset):
    """Colour input: the luminance kernel reads the caller's pitch (bytes) and writes its own
    aligned float buffer, which the pyramid then takes as aligned f32 input."""
    dense = IL.color_images(fmt)
    n, h, w, _ = dense.shape
    gray = [O.gray_from_color(im, fmt) for im in dense]
    feats, _ = _reference(("color", fmt), None, default_options(), gray)
    buf = IL.pad(dense, stride)
    if offset is None:
        _run_forms(gpu_ctx, lambda: gpu_ctx.extract_color(buf, fmt, stride=stride, shape=(n, h, w)),
                   feats, None, "aligned", False, f"host {fmt} {stride}", FORMS)
    else:
        with devmem.uploaded(buf, offset) as ptr:
            _run_forms(gpu_ctx,
                       lambda: gpu_ctx.extract_color(ptr, fmt, shape=(n, h, w, stride), device_ptr=True),
                       feats, None, "aligned", False, f"device {fmt} {stride} + {offset}", FORMS)


FIRST_OCTAVE = [dict(octave_min=1, preprocess_on_cpu=1), dict(octave_min=1, preprocess_on_cpu=0),
                dict(octave_min=-1)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("stride", [205, 208])
@pytest.mark.parametrize("over", FIRST_OCTAVE, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_first_octave_resampling(gpu_ctx, over, stride, device):
    """-fo != 0: k_input_down / k_input_up read the caller's pitch; the first level then reads
    the library's resampled buffer."""
    n, w, h = IL.SHAPES["A"]
    dense = IL.images("A")
    opts = default_options(**over)
    feats, levels = _reference("A", dense, opts)
    buf = IL.pad(dense, stride)
    shipped = FORMS[:1]
    if device:
        for offset in (0, 1):
            with devmem.uploaded(buf, offset) as ptr:
                _run_forms(gpu_ctx,
                           lambda: gpu_ctx.extract(ptr, shape=(n, h, w, stride), device_ptr=True),
                           feats, levels, None, True, f"device {over} {stride} + {offset}", shipped, opts)
    else:
        _run_forms(gpu_ctx, lambda: gpu_ctx.extract(buf, shape=(n, h, w), stride=stride), feats,
                   levels, None, True, f"host {over} {stride}", shipped, opts)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("stride", [205, 208])
def test_extract_stream(gpu_ctx, stride, pinned):
    n, w, h = IL.SHAPES["A"]
    dense = IL.images("A")
    feats, _ = _reference("A", dense, default_options())
    order = [0, 1, 1, 2]   # two batches of two images
    want = [feats[i] for i in order]
    bufs = [IL.pad(dense[0:2], stride), IL.pad(dense[1:3], stride)]
    pins = []
    if pinned:
        pins = [sgpu.PinnedArray(b.shape, np.uint8) for b in bufs]
        for p, b in zip(pins, bufs):
            p.array[...] = b
        bufs = [p.array for p in pins]
    gpu_ctx.set_options(default_options())
    try:
        for exact in (False, True):
            gpu_ctx.set_debug_flags(C.DEBUG_EXACT_DESCRIPTOR if exact else 0)
            k, d, counts = gpu_ctx.extract_stream(bufs, cap=4096, stride=stride, shape=(2, h, w))
            assert counts.tolist() == [len(rk) for rk, _ in want]
            rk = np.concatenate([f[0] for f in want])
            rd = np.concatenate([f[1] for f in want])
            assert k.shape == rk.shape and np.array_equal(_bits(k), _bits(rk))
            if exact:
                assert np.array_equal(_bits(d), _bits(rd))
            else:
                assert np.linalg.norm(d.astype(np.float64) - rd, axis=1).max() < DESC_L2_TOL
    finally:
        gpu_ctx.set_debug_flags(0)
        for p in pins:
            p.free()


@pytest.mark.parametrize("scale,shift", [(255.0, 0.0), (1.0, -0.5)], ids=["0..255", "-0.5..0.5"])
def test_f32_caller_range(gpu_ctx, scale, shift):
    """A caller's float image outside [0, 1]: float input takes the descriptor narrowing that
    does not rely on unit-range gradients (unit_input = 0)."""
    from sift_synth import synth_image
    img = (synth_image(200, 96, 77).astype(np.float32) / np.float32(255.0) * np.float32(scale)
           + np.float32(shift)).astype(np.float32)
    assert img.min() >= shift and img.max() <= scale + shift and img.max() - img.min() > 0.5 * scale
    rk, rd = O.extract_f32(img)
    assert len(rk) > 0
    _run_forms(gpu_ctx, lambda: gpu_ctx.extract(img), [(rk, rd)], None, None, False,
               f"f32 x {scale} + {shift}", FORMS[:1])
