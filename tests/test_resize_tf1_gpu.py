"""``asep_prep_resize_tf1[_dev]`` (csrc/post_kernels.h prep_resize_tf1_kernel) against the host function it replaces,
``gnn_input.resize_bilinear_tf1``, and against Pillow's ``convert('L')`` for the luma mode.  Every comparison is bit for bit
(``view(np.uint32)`` equal): the kernel restates the host's float32 sequence product by product, so there is no tolerance to choose."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _random_u8(rng, shape):
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    flat = a.reshape(-1)
    flat[0] = 0                                              # both ends of the range are always present
    flat[-1] = 255
    return a


def _host(image, h, w):
    from citlab_article_separation_new_amd import gnn_input
    return gnn_input.resize_bilinear_tf1(image, h, w)


def test_one_column_and_one_row_sweep_every_size_pair_up_to_24():
    """[H,1] -> [h,1] for every H, h in 1..24 and the transposed [1,W] -> [1,w]: ratio 1 and 2 (taps on integers), non-terminating
    ratios (10 to 3), upscaling with the clamp at the last row, 1-pixel sources"""
    from citlab_article_separation_new_amd import image_ops
    rng = np.random.default_rng(20261019)
    bad = []
    for n_in in range(1, 25):
        col = _random_u8(rng, (n_in, 1)) if n_in > 1 else np.array([[rng.integers(0, 256)]], np.uint8)
        row = np.ascontiguousarray(col.T)
        for n_out in range(1, 25):
            if not _bits_equal(image_ops.resize_tf1(col, n_out, 1)[:, :, 0], _host(col, n_out, 1)[:, :, 0]):
                bad.append(("column", n_in, n_out))
            if not _bits_equal(image_ops.resize_tf1(row, 1, n_out)[:, :, 0], _host(row, 1, n_out)[:, :, 0]):
                bad.append(("row", n_in, n_out))
    assert not bad, bad[:20]


def _two_dimensional_cases():
    from citlab_article_separation_new_amd import gnn_input
    cases = [((2, 3), (5, 7)), ((7, 5), (3, 2))]
    for hw in ((13, 45), (97, 131), (300, 451)):
        for lo, hi in ((8, 16), (64, 96), (256, 1024)):
            cases.append((hw, gnn_input.compute_new_size(hw[0], hw[1], lo, hi)))
    return cases


@pytest.mark.parametrize("channels", [1, 3])
def test_two_dimensional_pages_keep_mode(channels):
    from citlab_article_separation_new_amd import image_ops
    rng = np.random.default_rng(7 + channels)
    for (H, W), (h, w) in _two_dimensional_cases():
        a = _random_u8(rng, (H, W, channels))
        got = image_ops.resize_tf1(a, h, w)
        assert got.shape == (h, w, channels)
        assert _bits_equal(got, _host(a, h, w)), ((H, W, channels), (h, w))
        if channels == 1:                                    # a [H,W] page is the same page
            assert _bits_equal(image_ops.resize_tf1(a[:, :, 0], h, w), got)


def test_a_mid_size_colour_page_to_its_default_size():
    from citlab_article_separation_new_amd import gnn_input, image_ops
    a = _random_u8(np.random.default_rng(3), (1201, 803, 3))
    p = gnn_input.DEFAULT_INPUT_PARAMS
    h, w = gnn_input.compute_new_size(1201, 803, p["resize_min_dim"], p["resize_max_dim"])
    assert _bits_equal(image_ops.resize_tf1(a, h, w), _host(a, h, w))


def test_luma_of_every_rgb_triple_equals_pillows_convert_l():
    """a 4096 x 4096 page holding every R, G, B triple once, resized to its own size: scale 1, weights 0 -> the luma itself"""
    from PIL import Image
    from citlab_article_separation_new_amd import image_ops
    v = np.arange(1 << 24, dtype=np.uint32)
    a = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    want = np.asarray(Image.fromarray(a, "RGB").convert("L")).astype(np.float32)
    got = image_ops.resize_tf1(a, 4096, 4096, mode="luma")
    assert got.shape == (4096, 4096, 1)
    assert _bits_equal(got[:, :, 0], want)


def test_luma_then_resize_equals_the_host_resize_of_pillows_gray():
    from PIL import Image
    from citlab_article_separation_new_amd import gnn_input, image_ops
    a = _random_u8(np.random.default_rng(11), (97, 131, 3))
    gray = np.asarray(Image.fromarray(a, "RGB").convert("L"))
    h, w = gnn_input.compute_new_size(97, 131, 64, 96)
    assert _bits_equal(image_ops.resize_tf1(a, h, w, mode="luma")[:, :, 0], _host(gray, h, w)[:, :, 0])


@pytest.mark.parametrize("mode,channels", [("keep", 1), ("keep", 3), ("luma", 3)])
def test_device_entry_gives_the_bits_of_the_host_pointer_entry(mode, channels):
    import torch
    from citlab_article_separation_new_amd import image_ops
    a = _random_u8(np.random.default_rng(5), (97, 131, channels))
    host = image_ops.resize_tf1(a, 64, 87, mode)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = image_ops.resize_tf1_dev(torch.from_numpy(a).cuda(), 64, 87, mode)
    stream.synchronize()
    assert _bits_equal(dev.cpu().numpy(), host)


def test_refused_arguments_return_an_error_code_and_name_the_argument():
    from citlab_article_separation_new_amd import _lib, image_ops
    lib, ws = image_ops._workspace(0)
    a = np.zeros((4, 5, 3), np.uint8)
    out = np.zeros((4, 5, 3), np.float32)
    ip, op = a.ctypes.data, out.ctypes.data
    cases = [                                                # (p, img, H, W, C, mode, h, w, out) -> the words the message must hold
        ((None, ip, 4, 5, 3, 0, 4, 5, op), "handle"),
        ((ws, None, 4, 5, 3, 0, 4, 5, op), "img"),
        ((ws, ip, 4, 5, 3, 0, 4, 5, None), "out"),
        ((ws, ip, 4, 5, 2, 0, 4, 5, op), "C must be 1 or 3 (got 2)"),
        ((ws, ip, 4, 5, 4, 0, 4, 5, op), "C must be 1 or 3 (got 4)"),
        ((ws, ip, 4, 5, 1, 1, 4, 5, op), "luma reads C = 3"),
        ((ws, ip, 4, 5, 3, 2, 4, 5, op), "mode must be"),
        ((ws, ip, 0, 5, 3, 0, 4, 5, op), "source size H x W = 0 x 5"),
        ((ws, ip, 4, -1, 3, 0, 4, 5, op), "source size H x W = 4 x -1"),
        ((ws, ip, 4, 5, 3, 0, 0, 5, op), "target size h x w = 0 x 5"),
        ((ws, ip, 4, 5, 3, 0, 4, -2, op), "target size h x w = 4 x -2"),
    ]
    for args, words in cases:
        for name, extra in (("asep_prep_resize_tf1", ()), ("asep_prep_resize_tf1_dev", (None,))):
            rc = getattr(lib, name)(*args, *extra)           # (refused before anything is read: host addresses do for the _dev form)
            msg = _lib.last_error()
            assert rc == -1, (name, args, rc)                # ASEP_ERR_ARG
            assert name + ":" in msg and words in msg, (name, words, msg)
    assert C.c_int(lib.asep_prep_resize_tf1(ws, ip, 4, 5, 3, 0, 4, 5, op)).value == 0       # the accepted call next to them
