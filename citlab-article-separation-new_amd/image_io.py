"""Image file decode for the two ARU-Net pipelines (host side, Pillow instead of ``cv2.imread``).

    load_image_bgr          cv2.imread(path)                         helper:29   (8-bit, BGR channel order)
    load_image_gray         cv2.imread(path, IMREAD_GRAYSCALE)       swt_dist_trafo.py:19
    get_image_dimensions    image_stats.py:23-29                     (width, height)
    load_and_scale_image    helper:28-33                             decode here, scale + gray on the GPU
    load_jpeg_coefficients  (no counterpart)                         baseline JPEG: Huffman decode only, csrc/host_jpeg.c
    jpeg_page_to_device     (no counterpart)                         ... its pixels on the GPU, csrc/jpeg_engine.hip
    load_jpeg_scan          (no counterpart)                         baseline JPEG: stuffing and markers removed only, csrc/host_jpeg.c
    jpeg_scan_to_device     (no counterpart)                         ... Huffman decode and pixels on the GPU, csrc/jpeg_huffman_kernels.h

Grayscale files are kept single-channel: ``cv2.imread`` would replicate the channel three times and BGR2GRAY of
equal channels returns the value itself (3735 + 19235 + 9798 = 2^15), so the net input is identical.
JPEG decoders differ between libjpeg builds by +-1 in places; PNG / TIFF inputs are bit-identical.

``--device_jpeg True`` of run_net_post_processing splits a baseline JPEG's decode: only the Huffman decode stays on a CPU
(``load_jpeg_coefficients``), dequantisation, inverse DCT, chroma upsampling and colour conversion run on the device
(``jpeg_page_to_device``) and give the bytes Pillow with libjpeg-turbo gives; every file that path refuses (progressive,
CMYK, an orientation to apply, other samplings, damaged streams ...) is decoded by ``load_image_bgr`` as before.
"""
import ctypes as C
import os
import struct
import threading
import zlib

import numpy as np
from PIL import Image, ImageOps

from . import image_ops

Image.MAX_IMAGE_PIXELS = None        # newspaper scans exceed Pillow's decompression-bomb guard


def get_image_dimensions(image_path):
    with Image.open(image_path) as im:
        return im.size


_DEEP_GRAY = ("I;16", "I;16L", "I;16B", "I;16N", "I")      # Pillow modes of 16-bit (and wider) single-channel files


# ---- plain 8-bit PNG scans: zlib + un-filtering in C (csrc/host_png.c), everything else through Pillow -------------------------
_HOST_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libasep_host.so")
_host = None


def _host_lib():
    """libasep_host.so (include/asep_host.h), or False if it has not been built: the decode then stays with Pillow"""
    global _host
    if _host is None:
        try:
            lib = C.CDLL(_HOST_LIB)
            lib.asep_png_unfilter.restype = C.c_long
            lib.asep_png_unfilter.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p]
            lib.asep_rgb_to_bgr.restype = None
            lib.asep_rgb_to_bgr.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
            _host = lib
        except OSError:
            _host = False
    return _host


_host_jpeg = None


def _host_jpeg_lib():
    """libasep_host.so with the JPEG entry points bound, or False: a library built before they existed still serves the PNG path"""
    global _host_jpeg
    if _host_jpeg is None:
        lib = _host_lib()
        try:
            if not lib:
                raise AttributeError
            lib.asep_jpeg_probe.restype = C.c_int
            lib.asep_jpeg_probe.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
            lib.asep_jpeg_entropy_decode.restype = C.c_int
            lib.asep_jpeg_entropy_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
            _host_jpeg = lib
        except AttributeError:
            _host_jpeg = False
    return _host_jpeg


_deflate = None
_deflate_state = threading.local()


def _inflate(stream, nbytes):
    """zlib stream -> uint8 array of exactly ``nbytes``, valid until the calling thread's next call (None if the stream is damaged
    or has another length): libdeflate when the system
    has it (libdeflate.so.0 ships with this image; about twice the speed of zlib's inflate on scan data), else zlib"""
    global _deflate
    if _deflate is None:
        try:
            lib = C.CDLL("libdeflate.so.0")
            lib.libdeflate_alloc_decompressor.restype = C.c_void_p
            lib.libdeflate_zlib_decompress.restype = C.c_int
            lib.libdeflate_zlib_decompress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                       C.POINTER(C.c_size_t)]
            _deflate = lib
        except (OSError, AttributeError):
            _deflate = False
    if _deflate:
        d = getattr(_deflate_state, "d", None)
        if d is None:
            d = _deflate_state.d = _deflate.libdeflate_alloc_decompressor()     # one per thread, kept for the process's life
        if d:
            out = getattr(_deflate_state, "buf", None)       # scratch of the calling thread, reused from scan to scan (the
            if out is None or out.size != nbytes:            # caller un-filters out of it at once and keeps no reference)
                out = _deflate_state.buf = np.empty(nbytes, dtype=np.uint8)
            got = C.c_size_t(0)
            rc = _deflate.libdeflate_zlib_decompress(d, stream, len(stream), out.ctypes.data, nbytes, C.byref(got))
            if rc == 0 and got.value == nbytes:
                return out
            if rc in (1, 2):                                # LIBDEFLATE_BAD_DATA, SHORT_OUTPUT: not the image the header announces
                return None
            # (3 = INSUFFICIENT_SPACE: more data than announced -- zlib below agrees or refuses)
    try:
        data = zlib.decompress(stream)
    except zlib.error:
        return None
    return np.frombuffer(data, dtype=np.uint8) if len(data) == nbytes else None


_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
# ancillary chunks that change what cv2.imread / Pillow hand out (transparency, orientation): such files go through Pillow
_PNG_NOT_PLAIN = (b"tRNS", b"eXIf", b"PLTE", b"acTL")
# text chunks whose keyword starts like this carry an EXIF / XMP profile (ImageMagick's "Raw profile type exif", Adobe's XMP packet)
_PNG_TEXT_NOT_PLAIN = (b"Raw profile type", b"XML:com.adobe.xmp")


def _load_png_plain(path):
    """8-bit gray or RGB, non-interlaced PNG -> uint8 [H,W] or [H,W,3] BGR, exactly what Pillow decodes; None for every other
    flavour (palette, alpha, 16 bit, interlaced, transparency / EXIF chunks, damaged files -- Pillow reports those)."""
    lib = _host_lib()
    if not lib:
        return None
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != _PNG_SIGNATURE or len(raw) < 33 or raw[12:16] != b"IHDR":
        return None
    if zlib.crc32(raw[12:29]) & 0xffffffff != struct.unpack(">I", raw[29:33])[0]:
        return None                                         # damaged header: Pillow reports it (the pixel data carries zlib's own
                                                            # Adler-32, which the inflate step verifies)
    width, height, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", raw[16:29])
    if depth != 8 or colour not in (0, 2) or compression or filt or interlace or not width or not height:
        return None
    # a header may announce any size: Pillow's decompression-bomb limit applies here too (beyond it Pillow itself reports the file),
    # and a deflate stream expands at most ~1032x, so a size the file cannot possibly hold is a damaged or crafted header
    bpp = 1 if colour == 0 else 3
    stride = width * bpp
    limit = Image.MAX_IMAGE_PIXELS
    if (limit is not None and width * height > limit) or height * (stride + 1) > 1040 * len(raw):
        return None
    pos, parts = 8, []
    while pos + 12 <= len(raw):
        length, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        if kind in _PNG_NOT_PLAIN:
            return None
        if kind in (b"tEXt", b"zTXt", b"iTXt") and raw[pos + 8:pos + 8 + length].startswith(_PNG_TEXT_NOT_PLAIN):
            return None                                     # orientation / metadata profiles in text chunks: Pillow applies them
        if kind == b"IDAT":
            if zlib.crc32(raw[pos + 4:pos + 8 + length]) & 0xffffffff != struct.unpack(">I", raw[pos + 8 + length:pos + 12 + length] or b"\0\0\0\0")[0]:
                return None                                 # damaged chunk: Pillow reports it
            parts.append(raw[pos + 8:pos + 8 + length])
        elif kind == b"IEND":
            break
        pos += 12 + length
    if not parts:
        return None
    try:
        data = _inflate(parts[0] if len(parts) == 1 else b"".join(parts), height * (stride + 1))
        if data is None:
            return None
        out = np.empty((height, width) if bpp == 1 else (height, width, 3), dtype=np.uint8)
        if bpp == 1:
            rc = lib.asep_png_unfilter(data.ctypes.data, height, stride, 1, out.ctypes.data)
        else:
            rgb = np.empty((height, width, 3), dtype=np.uint8)
            rc = lib.asep_png_unfilter(data.ctypes.data, height, stride, 3, rgb.ctypes.data)
            if rc == 0:
                lib.asep_rgb_to_bgr(rgb.ctypes.data, height * width, out.ctypes.data)
    except MemoryError:                                     # let Pillow report what it makes of the file
        return None
    return out if rc == 0 else None


# ---- baseline JPEG scans: Huffman decode in C (csrc/host_jpeg.c), pixels on the device (csrc/jpeg_engine.hip) ------------------------
class JpegInfo(C.Structure):
    """asep_jpeg_info (include/asep_host.h)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("mcus_w", C.c_int32), ("mcus_h", C.c_int32), ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3),
                ("qt_index", C.c_int32 * 3), ("restart_interval", C.c_int32), ("reserved", C.c_int32), ("coef_bytes", C.c_int64)]


_JPEG_MAGIC = b"ASEPJPG1"
_JPEG_HEAD = 640                     # magic, JpegInfo, the four tables, padding: the coefficients start 128-byte aligned


class JpegPage:
    """The entropy-decoded half of a JPEG scan in ONE uint8 buffer (``packed``: what a decode worker puts into its page-locked
    slot): the frame description, the quantisation tables (uint16 [4, 64], natural order) and the quantised coefficients
    (int16, per component [blocks_h, blocks_w, 64] in natural order, DC prediction undone).  Views, no copies."""

    def __init__(self, packed):
        self.packed = packed
        self.info = JpegInfo.from_buffer(packed, len(_JPEG_MAGIC))
        self.qt = packed[8 + C.sizeof(JpegInfo):8 + C.sizeof(JpegInfo) + 512].view(np.uint16).reshape(4, 64)
        self.coef = packed[_JPEG_HEAD:_JPEG_HEAD + self.info.coef_bytes].view(np.int16)

    width = property(lambda self: self.info.width)
    height = property(lambda self: self.info.height)
    ncomp = property(lambda self: self.info.ncomp)
    hs = property(lambda self: self.info.hs)
    vs = property(lambda self: self.info.vs)
    qt_index = property(lambda self: list(self.info.qt_index)[:self.info.ncomp])

    def components(self):
        """the coefficients per component: int16 [blocks_h, blocks_w, 64]"""
        out, off = [], 0
        for c in range(self.ncomp):
            n = self.info.blocks_h[c] * self.info.blocks_w[c] * 64
            out.append(self.coef[off:off + n].reshape(self.info.blocks_h[c], self.info.blocks_w[c], 64))
            off += n
        return out


def as_jpeg_page(image):
    """a JpegPage if ``image`` is one or the ``packed`` buffer of one (as it comes out of a decode slot), else None"""
    if isinstance(image, JpegPage):
        return image
    if isinstance(image, np.ndarray) and image.ndim == 1 and image.dtype == np.uint8 and image.size >= _JPEG_HEAD \
            and image[:8].tobytes() == _JPEG_MAGIC:
        return JpegPage(np.require(image, requirements=['C', 'W']))
    return None


def load_jpeg_coefficients(path):
    """A baseline JPEG (8-bit Huffman; gray, or YCbCr 4:4:4 / 4:2:2 / 4:2:0 in one scan, no orientation to apply) -> JpegPage; None
    for everything else -- not a JPEG, a flavour host_jpeg.c refuses (among them a block with more energy than 8-bit samples give, where libjpeg-turbo's 16-bit
    SIMD arithmetic and the device's would part), a damaged stream, libasep_host.so not built: such a file goes
    through ``load_image_bgr``, so no file decodes differently than without this path."""
    lib = _host_jpeg_lib()
    if not lib:
        return None
    try:
        with open(path, "rb") as f:
            if f.read(2) != b"\xff\xd8":
                return None
            raw = b"\xff\xd8" + f.read()
    except OSError:
        return None
    info = JpegInfo()
    if lib.asep_jpeg_probe(raw, len(raw), C.byref(info)) != 0:
        return None
    # a header may announce any size: the same sanity check as for PNG (Pillow's decompression-bomb limit; the probe has already refused a
    # frame with more blocks than the file's bytes could code)
    limit = Image.MAX_IMAGE_PIXELS
    if limit is not None and info.width * info.height > limit:
        return None
    try:
        packed = np.empty(_JPEG_HEAD + info.coef_bytes, dtype=np.uint8)
    except MemoryError:
        return None
    packed[:8] = np.frombuffer(_JPEG_MAGIC, dtype=np.uint8)
    packed[8:_JPEG_HEAD] = 0
    C.memmove(packed.ctypes.data + 8, C.byref(info), C.sizeof(info))
    page = JpegPage(packed)
    if lib.asep_jpeg_entropy_decode(raw, len(raw), C.byref(info), page.coef.ctypes.data, page.qt.ctypes.data) != 0:
        return None
    return page


def jpeg_page_to_device(page, device=0, order="bgr", stream=None, lane=0):
    """JpegPage -> uint8 torch tensor on ``device``, the bytes Pillow decodes: [H,W] for a one-component page whatever the order, else
    [H,W,3] for ``order`` "bgr" (``load_image_bgr``) / "rgb" (the relation net's page_u8), [H,W] for "gray" (``load_image_gray``).
    The coefficients are uploaded and the kernels queued on ``stream`` (a torch stream; None = the current one); ``page`` must stay
    valid until the upload has run.  ``lane``: the scratch arena (``image_ops._workspace``), one per stream."""
    import torch
    from . import _lib
    tdev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    lib, ws = image_ops._workspace(tdev.index or 0, lane)
    with torch.cuda.device(tdev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(tdev)):
        sp = C.c_void_p(torch.cuda.current_stream(tdev).cuda_stream)
        d_coef = torch.empty(page.coef.size, dtype=torch.int16, device=tdev)
        d_coef.copy_(torch.from_numpy(page.coef), non_blocking=True)
        shape = (page.height, page.width) if page.ncomp == 1 or order == "gray" else (page.height, page.width, 3)
        out = torch.empty(shape, dtype=torch.uint8, device=tdev)
        _lib.check(lib.asep_jpeg_pixels_dev(ws, C.byref(page.info), d_coef.data_ptr(), page.qt.ctypes.data, _lib.JPEG_ORDERS[order],
                                            out.data_ptr(), sp), "asep_jpeg_pixels_dev")
        d_coef.record_stream(torch.cuda.current_stream(tdev))
    global jpeg_device_pages
    jpeg_device_pages += 1
    return out


jpeg_device_pages = 0                # pages jpeg_page_to_device has queued in this process


def jpeg_device_launches():
    """the kernels the calling thread's last device JPEG call launched (asep_jpeg_last_launches)"""
    from . import _lib
    lib = _lib.load_library()
    buf = C.create_string_buffer(4096)
    lib.asep_jpeg_last_launches(buf, len(buf))
    return buf.value.decode().split()


# ---- baseline JPEG scans, entropy decode on the device as well (--device_huffman; csrc/jpeg_huffman_kernels.h) ------------------------------
class JpegHuff(C.Structure):
    """asep_jpeg_huff (include/asep_host_jpeg_scan.h)"""
    _fields_ = [("look", C.c_uint16 * 512), ("maxcode", C.c_int32 * 18), ("valoff", C.c_int32 * 18), ("sym", C.c_uint8 * 256),
                ("nsym", C.c_int32), ("reserved", C.c_int32)]


class JpegScanTables(C.Structure):
    """asep_jpeg_scan_tables"""
    _fields_ = [("dc", JpegHuff * 3), ("ac", JpegHuff * 3), ("qt", (C.c_uint16 * 64) * 4)]


JPEG_SEGMENT = np.dtype([("byte_offset", "<u4"), ("byte_length", "<u4"), ("first_mcu", "<u4"), ("n_mcus", "<u4")])   # asep_jpeg_segment
JPEG_STATUS_DAMAGED, JPEG_STATUS_REFUSED, JPEG_STATUS_NOT_CONVERGED = 1, 2, 4     # ASEP_JPEG_STATUS_* of include/asep_hip.h
_SCAN_MAGIC = b"ASEPJSC1"
_SCAN_TABLES = 128                   # magic, JpegInfo, scan_bytes, n_segments (two int64), padding; then the tables, the segments, the bytes
_SCAN_SEGMENTS = _SCAN_TABLES + C.sizeof(JpegScanTables)


class JpegScan:
    """A baseline JPEG scan prepared for the device's entropy decode, in ONE uint8 buffer (``packed``, as a decode worker puts it into
    its slot): the frame description, the Huffman and quantisation tables, the segments (restart intervals) and the entropy-coded
    bytes without stuffing and markers.  Views, no copies."""

    def __init__(self, packed):
        self.packed = packed
        self.info = JpegInfo.from_buffer(packed, len(_SCAN_MAGIC))
        counts = packed[8 + C.sizeof(JpegInfo):8 + C.sizeof(JpegInfo) + 16].view(np.int64)
        self.scan_bytes, self.n_segments = int(counts[0]), int(counts[1])
        self.tables = JpegScanTables.from_buffer(packed, _SCAN_TABLES)
        self.qt = packed[_SCAN_SEGMENTS - 512:_SCAN_SEGMENTS].view(np.uint16).reshape(4, 64)
        first = _SCAN_SEGMENTS + 16 * self.n_segments
        self.segments = packed[_SCAN_SEGMENTS:first].view(JPEG_SEGMENT)
        self.scan = packed[first:first + (self.scan_bytes + 3) // 4 * 4]       # whole 32-bit words, zeros behind the last byte

    width = property(lambda self: self.info.width)
    height = property(lambda self: self.info.height)
    ncomp = property(lambda self: self.info.ncomp)


def as_jpeg_scan(image):
    """a JpegScan if ``image`` is one or the ``packed`` buffer of one, else None"""
    if isinstance(image, JpegScan):
        return image
    if isinstance(image, np.ndarray) and image.ndim == 1 and image.dtype == np.uint8 and image.size >= _SCAN_SEGMENTS \
            and image[:8].tobytes() == _SCAN_MAGIC:
        return JpegScan(np.require(image, requirements=['C', 'W']))
    return None


def _host_scan_lib():
    """libasep_host.so with asep_jpeg_scan_prepare bound, or False"""
    lib = _host_jpeg_lib()
    if lib and not hasattr(lib, "_scan_bound"):
        try:
            lib.asep_jpeg_scan_sizes.restype = C.c_int
            lib.asep_jpeg_scan_sizes.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
            lib.asep_jpeg_scan_prepare.restype = C.c_int
            lib.asep_jpeg_scan_prepare.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_size_t, C.c_void_p, C.c_void_p]
            lib._scan_bound = True
        except AttributeError:
            lib._scan_bound = False
    return lib if lib and lib._scan_bound else False


def prepare_jpeg_scan(raw):
    """the bytes of a JPEG file -> (JpegScan, 0), or (None, the negative code of asep_jpeg_probe / asep_jpeg_scan_sizes / _prepare)"""
    lib = _host_scan_lib()
    if not lib:
        raise RuntimeError(f"{_HOST_LIB} is not built or does not export asep_jpeg_scan_prepare")
    info = JpegInfo()
    rc = lib.asep_jpeg_probe(raw, len(raw), C.byref(info))
    if rc != 0:
        return None, rc
    limit = Image.MAX_IMAGE_PIXELS                                   # as load_jpeg_coefficients
    if limit is not None and info.width * info.height > limit:
        return None, -1
    cap, nseg = C.c_size_t(), C.c_size_t()
    rc = lib.asep_jpeg_scan_sizes(C.byref(info), len(raw), C.byref(cap), C.byref(nseg))
    if rc != 0:
        return None, rc
    first = _SCAN_SEGMENTS + 16 * nseg.value
    packed = np.zeros(first + cap.value, dtype=np.uint8)
    used, got = C.c_size_t(), C.c_size_t()
    rc = lib.asep_jpeg_scan_prepare(raw, len(raw), C.byref(info), packed.ctypes.data + first, cap.value, C.byref(used),
                                    packed.ctypes.data + _SCAN_SEGMENTS, nseg.value, C.byref(got), packed.ctypes.data + _SCAN_TABLES)
    if rc != 0:
        return None, rc
    assert got.value == nseg.value and used.value <= cap.value
    packed[:8] = np.frombuffer(_SCAN_MAGIC, dtype=np.uint8)
    C.memmove(packed.ctypes.data + 8, C.byref(info), C.sizeof(info))
    packed[8 + C.sizeof(info):8 + C.sizeof(info) + 16].view(np.int64)[:] = (used.value, got.value)
    return JpegScan(packed[:first + (used.value + 3) // 4 * 4]), 0


def load_jpeg_scan(path):
    """A baseline JPEG -> JpegScan, after one pass over its markers and bytes; None where ``load_jpeg_coefficients`` returns None
    before its entropy decode (not a JPEG, a refused flavour, a damaged marker structure, libasep_host.so not built).  What only the
    entropy decode finds shows in the status of ``jpeg_scan_to_device``."""
    if not _host_scan_lib():
        return None
    try:
        with open(path, "rb") as f:
            if f.read(2) != b"\xff\xd8":
                return None
            raw = b"\xff\xd8" + f.read()
    except OSError:
        return None
    try:
        return prepare_jpeg_scan(raw)[0]
    except MemoryError:
        return None


def jpeg_scan_entropy_to_device(scan, device=0, stream=None, lane=0, subseq_bits=0):
    """JpegScan -> (int16 coefficients on the device, laid out as ``JpegPage.coef``; int32 status tensor [1] on the device).  The
    scan's bytes are uploaded and the entropy kernels queued on ``stream``; the call waits for the stream while the fixed-point
    loop reads its "changed" word (asep_jpeg_entropy_dev)."""
    import torch
    from . import _lib
    tdev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    lib, ws = image_ops._workspace(tdev.index or 0, lane)
    with torch.cuda.device(tdev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(tdev)):
        sp = C.c_void_p(torch.cuda.current_stream(tdev).cuda_stream)
        d_scan = torch.empty(scan.scan.size, dtype=torch.uint8, device=tdev)
        d_scan.copy_(torch.from_numpy(scan.scan), non_blocking=True)
        d_coef = torch.empty(scan.info.coef_bytes // 2, dtype=torch.int16, device=tdev)
        d_status = torch.empty(1, dtype=torch.int32, device=tdev)
        _lib.check(lib.asep_jpeg_entropy_dev(ws, C.byref(scan.info), d_scan.data_ptr(), scan.scan_bytes, C.byref(scan.tables),
                                             scan.segments.ctypes.data, scan.n_segments, int(subseq_bits), d_coef.data_ptr(),
                                             d_status.data_ptr(), sp), "asep_jpeg_entropy_dev")
        d_scan.record_stream(torch.cuda.current_stream(tdev))
    return d_coef, d_status


def jpeg_scan_to_device(scan, device=0, order="bgr", stream=None, lane=0, subseq_bits=0):
    """JpegScan -> (uint8 page tensor on ``device`` as ``jpeg_page_to_device`` returns it, int32 status tensor [1] on the device).
    The entropy kernels and then the pixel kernels are queued on ``stream``.  The page holds Pillow's bytes only where the status is 0:
    the caller reads it before the page is used and decodes the file through ``load_image_bgr_or_jpeg`` otherwise."""
    import torch
    from . import _lib
    tdev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    lib, ws = image_ops._workspace(tdev.index or 0, lane)
    with torch.cuda.device(tdev), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(tdev)):
        sp = C.c_void_p(torch.cuda.current_stream(tdev).cuda_stream)
        d_coef, d_status = jpeg_scan_entropy_to_device(scan, tdev, torch.cuda.current_stream(tdev), lane, subseq_bits)
        entropy_launches = jpeg_device_launches()
        shape = (scan.height, scan.width) if scan.ncomp == 1 or order == "gray" else (scan.height, scan.width, 3)
        out = torch.empty(shape, dtype=torch.uint8, device=tdev)
        _lib.check(lib.asep_jpeg_pixels_dev(ws, C.byref(scan.info), d_coef.data_ptr(), scan.qt.ctypes.data, _lib.JPEG_ORDERS[order],
                                            out.data_ptr(), sp), "asep_jpeg_pixels_dev")
        d_coef.record_stream(torch.cuda.current_stream(tdev))
    global jpeg_huffman_pages, _scan_launches
    jpeg_huffman_pages += 1
    _scan_launches = entropy_launches + jpeg_device_launches()
    return out, d_status


jpeg_huffman_pages = 0               # pages jpeg_scan_to_device has queued in this process
jpeg_huffman_fallbacks = 0           # ... of which a non-zero status sent the file back to the host decoders
_scan_launches = []


def jpeg_scan_launches():
    """the kernels of this process's last ``jpeg_scan_to_device``, entropy and pixels"""
    return list(_scan_launches)


def jpeg_entropy_rounds():
    """(rounds of the calling thread's last device entropy decode until a launch changed nothing, its subsequences)"""
    from . import _lib
    n = C.c_int()
    return _lib.load_library().asep_jpeg_entropy_last_rounds(C.byref(n)), n.value


def jpeg_entropy_set_max_rounds(max_rounds):
    """for tests: cap the rounds of the calling thread's later device entropy decodes (0 = the library's cap alone)"""
    from . import _lib
    _lib.load_library().asep_jpeg_entropy_set_max_rounds(int(max_rounds))


class DevicePage:
    """a page that is already on the device ([H, W] or [H, W, 3] uint8): what ``resolve_jpeg_scans`` puts in a JpegScan's place"""

    def __init__(self, d_img):
        self.d_img = d_img


def resolve_jpeg_scans(batch, device, stream=None, lane=0, order="bgr"):
    """[(path, image)] of a group of decoded pages -> the same list with every JpegScan (or its packed buffer) replaced: by a
    DevicePage where the device's entropy decode reports status 0, else by what ``load_image_bgr_or_jpeg(path)`` returns.  The
    statuses of the group are read together, once, before any of its pages is used."""
    import torch
    found = [(i, as_jpeg_scan(image)) for i, (_, image) in enumerate(batch)]
    found = [(i, s) for i, s in found if s is not None]
    if not found:
        return batch
    queued = [jpeg_scan_to_device(s, device, order, stream, lane) for _, s in found]
    status = torch.cat([st for _, st in queued]).cpu().numpy()
    out = list(batch)
    global jpeg_huffman_fallbacks
    for (i, _), (d_img, _), st in zip(found, queued, status):
        if st == 0:
            out[i] = (batch[i][0], DevicePage(d_img))
        else:
            jpeg_huffman_fallbacks += 1
            out[i] = (batch[i][0], load_image_bgr_or_jpeg(batch[i][0]))
    return out


def load_image_bgr_or_jpeg_scan(path_to_image):
    """DecodePool loader of ``--device_huffman True``: the ``packed`` buffer of a JpegScan where the device path takes the file, else
    what ``load_image_bgr`` returns"""
    scan = load_jpeg_scan(path_to_image)
    return scan.packed if scan is not None else load_image_bgr(path_to_image)


def load_image_bgr_or_jpeg(path_to_image):
    """DecodePool loader of ``--device_jpeg True``: the ``packed`` buffer of a JpegPage where the device path takes the file, else what
    ``load_image_bgr`` returns"""
    page = load_jpeg_coefficients(path_to_image)
    return page.packed if page is not None else load_image_bgr(path_to_image)


def load_image_bgr(path_to_image):
    """uint8 [H,W,3] in BGR order, or uint8 [H,W] for single-channel files.

    Like ``cv2.imread`` with its default flags: the EXIF orientation is applied, an alpha channel is dropped, palette
    files are expanded, and 16-bit samples are reduced to their high byte (libpng's ``strip_16``; Pillow's own
    ``convert('L')`` would clip everything above 255 to white instead)."""
    if str(path_to_image).lower().endswith(".png"):
        plain = _load_png_plain(path_to_image)
        if plain is not None:
            return plain
    with Image.open(path_to_image) as im:
        im = ImageOps.exif_transpose(im)
        if im.mode in _DEEP_GRAY:
            deep = np.asarray(im).astype(np.int64)
            return np.clip(deep >> 8, 0, 255).astype(np.uint8)
        if im.mode == "F":
            return np.clip(np.rint(np.asarray(im, dtype=np.float64)), 0, 255).astype(np.uint8)
        if im.mode in ("L", "1", "LA", "La"):
            return np.asarray(im if im.mode == "L" else im.convert("L"), dtype=np.uint8)
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def load_image_gray(path_to_image):
    """8-bit gray like ``cv2.imread(path, cv2.IMREAD_GRAYSCALE)``: colour files go through the BGR2GRAY weights
    (OpenCV converts inside the decoder; for PNG/TIFF that is the same fixed-point formula)."""
    img = load_image_bgr(path_to_image)
    if img.ndim == 2:
        return img
    b, g, r = (img[:, :, i].astype(np.int32) for i in range(3))
    return ((b * 3735 + g * 19235 + r * 9798 + 16384) >> 15).astype(np.uint8)


def load_and_scale_image(path_to_image, fixed_height, scaling_factor, device=0):
    """helper:28-33 -> (image uint8 scaled, image_grey float32 [h,w] in 0..1, sc)."""
    image = load_image_bgr(path_to_image)
    return image_ops.scale_and_gray(image, fixed_height, scaling_factor, device=device)
