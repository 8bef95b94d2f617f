"""JPEG files from the device encoder (ir_jpeg_encode, csrc/jpeg_encode.hip): the GPU produces the entropy-coded segment of a baseline JPEG -
colour conversion, chroma downsample, forward DCT, quantisation, Huffman coding with the standard (Annex K) tables, byte stuffing and restart
markers - and the host adds the headers around it, a few hundred bytes that depend on the size and the three parameters alone.

A baseline JPEG with the standard tables and a restart interval is a deterministic function of the pixels, so the file equals, byte for byte,
what PIL writes with Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_blocks=RESTART_MCUS): which encoder coded a file
never shows. tools/jpeg_encode_model.py is the definition both are tested against.
"""
import ctypes as C
import struct
from typing import List, Sequence, Tuple

# MCUs per restart interval, the one value the product uses: the host path passes it to PIL as restart_marker_blocks, the device path to the
# kernel, which codes one interval per workgroup. 16 by measured time of ir_jpeg_encode on a 2048 x 2048 result at quality 95 / 4:2:0 (1024
# intervals): 0.088 ms against 0.102 at 8, 0.108 at 32, 0.159 at 64 and 0.269 at 128 MCUs, for a file 0.2 % larger than at 32
# (profiles/jpeg_encoder.txt).
RESTART_MCUS = 16

SUBSAMPLINGS = (0, 2)   # PIL's numbers: 0 = 4:4:4, 2 = 4:2:0

_LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K.3's four tables as DHT payloads behind the class / id byte: 16 counts, then the symbols in code order
_DC_LUMA = bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + bytes(range(12))
_DC_CHROMA = bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]) + bytes(range(12))
_AC_LUMA = bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]) + bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]) + bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def subsampling_of(v) -> int:
    """PIL's number for a subsampling given as that number (0, 2) or as 444 / 420 / "4:4:4" / "4:2:0"."""
    names = {0: 0, 2: 2, 444: 0, 420: 2, "444": 0, "420": 2, "4:4:4": 0, "4:2:0": 2}
    if v not in names:
        raise ValueError("JPEG subsampling must be 4:2:0 (2, 420) or 4:4:4 (0, 444)")
    return names[v]


def check_params(quality: int, subsampling: int, restart_mcus: int = 1) -> None:
    if not 1 <= quality <= 100:
        raise ValueError("JPEG quality must be 1 .. 100")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError("JPEG subsampling must be 0 (4:4:4) or 2 (4:2:0)")
    if not 1 <= restart_mcus <= 65535:
        raise ValueError("the restart interval must be 1 .. 65535 MCUs")


def jpeg_header(width: int, height: int, quality: int, subsampling: int, restart_mcus: int) -> bytes:
    """Everything in front of the entropy-coded segment, in PIL's (libjpeg's) order: SOI, APP0 (JFIF 1.01, no units, density 1 x 1), the two
    DQT of jpeg_set_quality(quality, force_baseline) in zigzag order, SOF0, the four DHT, DRI, SOS."""
    check_params(quality, subsampling, restart_mcus)
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError("a JPEG's sides are 1 .. 65535")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    parts = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for i, base in enumerate((_LUMA_Q, _CHROMA_Q)):
        table = [min(max((base[k] * scale + 50) // 100, 1), 255) for k in _ZIGZAG]
        parts.append(_segment(0xDB, bytes([i]) + bytes(table)))
    y_sampling = 0x22 if subsampling == 2 else 0x11
    parts.append(_segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, y_sampling, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, table in ((0x00, _DC_LUMA), (0x10, _AC_LUMA), (0x01, _DC_CHROMA), (0x11, _AC_CHROMA)):
        parts.append(_segment(0xC4, bytes([tc_th]) + table))
    parts.append(_segment(0xDD, struct.pack(">H", restart_mcus)))
    parts.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(parts)


def wrap_jpeg(entropy, width: int, height: int, quality: int, subsampling: int, restart_mcus: int) -> bytes:
    """The JPEG file (baseline, 8-bit YCbCr, JFIF, no other metadata - what PIL writes for mode RGB) around an entropy-coded segment."""
    if len(entropy) < 1:
        raise ValueError("wrap_jpeg: empty segment")
    return b"".join([jpeg_header(width, height, quality, subsampling, restart_mcus), entropy, b"\xff\xd9"])


def save_host(image, path_or_file, quality: int, subsampling: int, restart_mcus: int = RESTART_MCUS) -> None:
    """The host encoder: PIL with the parameters that make its file the device encoder's."""
    check_params(quality, subsampling, restart_mcus)
    image.save(path_or_file, format="JPEG", quality=quality, subsampling=subsampling, restart_marker_blocks=restart_mcus)


def bound(h: int, w: int, subsampling: int, restart_mcus: int = RESTART_MCUS) -> int:
    """ir_jpeg_bound: bytes that hold the entropy-coded segment of any h x w image at any quality."""
    from . import _lib as L
    return int(L.load_library().ir_jpeg_bound(h, w, subsampling, restart_mcus))


class JpegEncoder:
    """Device and page-locked host buffers for the segments of up to `count` images of at most h x w pixels, and the calls around them:
    queue() puts ir_jpeg_encode for a batch on the current stream, fetch_sizes() / fetch() bring back the byte counts and then only the
    bytes produced. One instance per batch shape, parameters and staging slot (pipeline.process_stream keeps them on the context)."""

    def __init__(self, ctx, count: int, h: int, w: int, quality: int = 95, subsampling: int = 2, restart_mcus: int = RESTART_MCUS):
        import torch
        check_params(quality, subsampling, restart_mcus)
        self.ctx, self.count, self.h, self.w = ctx, count, h, w
        self.quality, self.subsampling, self.restart_mcus = quality, subsampling, restart_mcus
        self.stride = (bound(h, w, subsampling, restart_mcus) + 255) & ~255
        self.d_out = torch.empty((count, self.stride), dtype=torch.uint8, device=ctx.device)
        self.d_info = torch.zeros(count, dtype=torch.int32, device=ctx.device)
        self.h_out = torch.empty((count, self.stride), dtype=torch.uint8).pin_memory()
        self.h_info = torch.zeros(count, dtype=torch.int32).pin_memory()
        self.rects: List[Tuple[int, int]] = [(h, w)] * count

    def queue(self, first: int, images, rects: Sequence[Tuple[int, int]]) -> None:
        """Encode the valid rectangles rects[i] = (vh, vw) of images [n][h][w][3] (device uint8) into slots first .. first + n - 1, on the current
        stream. Images of one rectangle share a call; the scratch is the context's workspace (the calls are stream-ordered)."""
        from . import _lib as L
        n, h, w, _ = images.shape
        if len(rects) != n or first + n > self.count or h > self.h or w > self.w:
            raise ValueError("JpegEncoder.queue: batch does not fit the buffers")
        ctx = self.ctx
        i = 0
        while i < n:
            k = i + 1
            while k < n and tuple(rects[k]) == tuple(rects[i]):
                k += 1
            vh, vw = (int(v) for v in rects[i])
            ws = ctx.workspace(ctx.ws_bytes(L.STAGE_JPEG, k - i, vh, vw, self.subsampling, self.restart_mcus))
            ctx.check(ctx.lib.ir_jpeg_encode(ctx.h, ctx.stream(), C.c_void_p(images[i].data_ptr()), k - i, h, w, 3 * w, vh, vw,
                                             self.quality, self.subsampling, self.restart_mcus,
                                             C.c_void_p(self.d_out[first + i].data_ptr()), self.stride, C.c_void_p(self.d_info[first + i].data_ptr()),
                                             L.ptr(ws), ws.numel()), "ir_jpeg_encode")
            for j in range(i, k):
                self.rects[first + j] = (vh, vw)
            i = k

    def fetch_sizes(self) -> None:
        """Asynchronous download of the byte counts on the current stream."""
        self.h_info.copy_(self.d_info, non_blocking=True)

    def fetch(self, used: int, stream=None, wrap: bool = True) -> list:
        """After fetch_sizes() has completed: download the produced bytes of slots 0 .. used - 1 on `stream` (default: the current one), wait, and
        return the JPEG files - or, with wrap=False, (segment, width, height, quality, subsampling, restart_mcus) tuples for a later
        wrap_jpeg(*pieces) on another thread."""
        import torch
        stream = stream or torch.cuda.current_stream(self.ctx.device)
        sizes = [int(v) for v in self.h_info[:used].tolist()]
        with torch.cuda.stream(stream):
            for i, size in enumerate(sizes):
                if not 0 < size <= self.stride:
                    raise RuntimeError(f"ir_jpeg_encode reported {size} bytes for a slot of {self.stride}")
                self.h_out[i, :size].copy_(self.d_out[i, :size], non_blocking=True)
        stream.synchronize()
        host = self.h_out.numpy()
        pieces = [(host[i, :size].tobytes(), self.rects[i][1], self.rects[i][0], self.quality, self.subsampling, self.restart_mcus)
                  for i, size in enumerate(sizes)]
        return pieces if not wrap else [wrap_jpeg(*p) for p in pieces]
