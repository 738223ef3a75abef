"""The padded input layouts of input_layouts.py (CPU only): every layout the GPU tests of
test_gpu_input_layout.py run compacts back to the dense images, and can show the two faults the
GPU tests are there to catch -- a reader that steps rows by the width instead of the pitch, and a
filter that clamps to the pitch instead of the width -- as a different oracle level (0, 0).  A
layout that could not show them would prove nothing on the device."""
import numpy as np
import pytest

import input_layouts as IL
import oracle_py as O

_images, _color = IL.images, IL.color_images


def _level00(img):
    h = img.shape[0]
    return O.gaussian(img, 0, 0).reshape(h, -1)


U8_STRIDES = sorted({(s, st) for s, st, _ in IL.U8_LAYOUTS})


@pytest.mark.parametrize("shape,stride", U8_STRIDES)
def test_u8_layout_compacts_and_shows_both_faults(shape, stride):
    imgs = _images(shape)
    n, w, h = IL.SHAPES[shape]
    tw = w & ~3
    buf = IL.pad(imgs, stride)
    assert buf.shape == (n * h * stride,) and buf.dtype == np.uint8
    assert np.array_equal(IL.compact(buf, imgs.shape, stride), imgs)
    pad_cols = buf.reshape(n, h, stride)[:, :, w:]
    assert np.array_equal(pad_cols, np.broadcast_to(IL.poison(np.uint8, h, stride - w, w), pad_cols.shape))
    if stride == w:
        return   # the control: rows w apart, as every other GPU test has them
    assert set(np.unique(pad_cols)) <= {0, 255}
    for image in (0, n - 1):
        right = _level00(imgs[image])
        assert right.shape == (h, tw)
        wrong_pitch = _level00(IL.misread_pitch(buf, imgs.shape, stride, image))
        assert wrong_pitch.shape == right.shape and not np.array_equal(wrong_pitch, right)
        wrong_clamp = _level00(IL.misread_clamp(buf, imgs.shape, stride, image))[:, :tw]
        assert not np.array_equal(wrong_clamp, right)
        # the clamp fault touches only what the filter reaches from the right edge
        assert np.array_equal(wrong_clamp[:, :tw - 16], right[:, :tw - 16]) or tw <= 16


@pytest.mark.parametrize("stride", sorted({st for _, st, _ in IL.F32_LAYOUTS}))
def test_f32_layout_compacts_and_poisons_with_nan(stride):
    n, w, h = IL.SHAPES["A"]
    imgs = _images("A").astype(np.float32) / np.float32(255.0)
    buf = IL.pad(imgs, stride)
    assert buf.shape == (n * h * stride,) and buf.dtype == np.float32
    assert np.array_equal(IL.compact(buf, imgs.shape, stride), imgs)
    assert np.isnan(buf.reshape(n, h, stride)[:, :, w:]).all() and not np.isnan(imgs).any()
    if stride == w:
        return
    # the index mapping is the u8 layout's of the same stride (checked above through the oracle);
    # here: both faults bring NaN into the columns a level reads
    tw = w & ~3
    for image in (0, n - 1):
        assert np.isnan(IL.misread_pitch(buf, imgs.shape, stride, image)[:, :tw]).any()
        assert np.isnan(IL.misread_clamp(buf, imgs.shape, stride, image)[:, tw:tw + 6]).any()


@pytest.mark.parametrize("fmt,stride", IL.COLOR_LAYOUTS)
def test_color_layout_compacts_and_shows_wrong_pitch(fmt, stride):
    imgs = _color(fmt)
    n, h, w, ch = imgs.shape
    buf = IL.pad(imgs, stride)
    assert buf.shape == (n * h * stride,)
    assert np.array_equal(IL.compact(buf, imgs.shape, stride), imgs)
    if stride == w * ch:
        return
    for image in (0, n - 1):
        right = O.extract_f32(O.gray_from_color(imgs[image], fmt))[0]
        wrong = O.extract_f32(O.gray_from_color(IL.misread_pitch(buf, imgs.shape, stride, image), fmt))[0]
        assert len(right) > 0
        assert wrong.shape != right.shape or not np.array_equal(wrong, right)


def test_wrapper_takes_the_buffer_the_library_will_read():
    """SiftContext's argument handling (no device): a strided call must pass a buffer that holds
    the n * h * stride elements the library copies, and the dense default stays rows w apart."""
    import sgpu
    padded = sgpu.SiftContext._padded
    imgs = _images("C")
    n, w, h = IL.SHAPES["C"]
    a, *dims = padded(imgs, None, None, np.uint8)
    assert dims == [n, h, w, w] and a.shape == imgs.shape
    assert padded(imgs[0], None, None, np.uint8)[1:] == (1, h, w, w)
    buf = IL.pad(imgs, 20)
    a, *dims = padded(buf, 20, (n, h, w), np.uint8)
    assert dims == [n, h, w, 20] and a.ctypes.data == buf.ctypes.data
    with pytest.raises(ValueError):
        padded(buf[:-1], 20, (n, h, w), np.uint8)     # the last row's padding is missing
    with pytest.raises(ValueError):
        padded(buf, 15, (n, h, w), np.uint8)          # rows overlap
    with pytest.raises(ValueError):
        padded(buf, 20, None, np.uint8)               # a flat buffer has no shape of its own
    color = _color("rgb")
    ch, cw = color.shape[1:3]
    assert padded(color, None, None, np.uint8, 3)[1:] == (2, ch, cw, cw * 3)
    with pytest.raises(ValueError):
        padded(color, None, None, np.uint8, 4)


def test_pad_rejects_a_short_stride():
    with pytest.raises(ValueError):
        IL.pad(_images("C"), 15)
