"""Frame sources and sinks for the host side of the motion loop.

The reference reads with cv2.VideoCapture (fm.py:413, 501) and writes the
motion frames with cv2.VideoWriter (fm.py:447-475).  Decode/encode stay on
the host (BASELINE.json north_star), so this module only adapts what is
available:

* OpenCV, when importable: cv2.VideoCapture / cv2.VideoWriter, as the
  reference does;
* otherwise (this image has no cv2): uncompressed RIFF AVI (BI_RGB, 24-bit
  BGR, bottom-up rows), read and written here -- the container OpenCV itself
  writes for fourcc 'DIB ' and reads through FFmpeg's rawvideo decoder;
* MJPEG AVI (fourcc 'MJPG', one baseline JPEG per '00dc' chunk): with OpenCV
  present, cv2.VideoCapture reads it as the reference does (fm.py:413) unless
  the caller opts in to the GPU decoder (gpu_decode=True, CLI --gpu-decode);
  without OpenCV it is read here.  MjpegAviCapture.read_jpeg() hands the
  compressed frames to the GPU decoder (find_motion_amd.MJpegDecoder /
  fm_submit_jpeg), so only compressed bytes cross PCIe.
  That decode is bit-exact to libjpeg-turbo's default decode, i.e. to
  cv2.imdecode and OpenCV's built-in MJPEG reader (CAP_OPENCV_MJPEG) -- not to
  cv2.VideoCapture's default FFmpeg backend (libavcodec's IDCT and swscale's
  colour conversion), whose frames may differ by a few levels (that parity is
  unpinned: neither FFmpeg nor OpenCV is in this image).  A stream the GPU
  decoder does not take (progressive, 12-bit, 4:1:1 ...) is decoded on the host
  instead (cv2.imdecode, else Pillow: libjpeg-turbo either way).
  MjpegAviWriter writes such files: the 'MJPG' output of an MJPEG input keeps
  the source's JPEG bytes (write_jpeg); write() encodes a BGR frame with
  Pillow, or -- on opt-in (open_writer(gpu_encode=True), CLI --gpu-encode) --
  on the GPU (find_motion_amd.MJpegEncoder), write_device() a frame already in
  HBM: the same bytes either way (libjpeg-turbo's, as Pillow writes them; not
  those of cv2.VideoWriter's own MJPG encoder, whose parity is unpinned);
* in-memory sources for tests, benchmarks and embedding: ArrayCapture over a
  [N][H][W][3] uint8 array and SyntheticCapture over the deterministic
  synthetic video of find_motion_amd.synthetic.

Every capture implements the subset of the cv2.VideoCapture protocol the
reference uses: isOpened(), read() -> (ok, frame), get(CAP_PROP_*), release().
"""
from __future__ import annotations

import logging
import os
import struct

import numpy as np

log = logging.getLogger("find_motion_amd.videoio")

try:  # pragma: no cover - OpenCV is not installed in the build image
    import cv2  # type: ignore
except Exception:  # noqa: BLE001
    cv2 = None

# cv2.CAP_PROP_* values (videoio.hpp)
CAP_PROP_FPS = 5
CAP_PROP_FRAME_WIDTH = 3
CAP_PROP_FRAME_HEIGHT = 4
CAP_PROP_FRAME_COUNT = 7


class ArrayCapture:
    """VideoCapture protocol over an in-memory uint8 array [N][H][W][3] (BGR)."""

    def __init__(self, frames, fps: float = 30.0):
        self._frames = frames
        self._i = 0
        self._open = True
        self._fps = float(fps)

    def isOpened(self) -> bool:  # noqa: N802 (cv2 protocol)
        return self._open

    def read(self):
        if not self._open or self._i >= len(self._frames):
            return False, None
        f = np.ascontiguousarray(self._frames[self._i], dtype=np.uint8)
        self._i += 1
        return True, f

    def get(self, prop: int) -> float:
        n = len(self._frames)
        if prop == CAP_PROP_FRAME_COUNT:
            return float(n)
        if n == 0:
            return 0.0
        shape = self._frames[0].shape
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(shape[1])
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(shape[0])
        if prop == CAP_PROP_FPS:
            return self._fps
        return 0.0

    def release(self) -> None:
        self._open = False


class JpegListCapture:
    """VideoCapture protocol over in-memory JPEG frames (an MJPEG stream already split into frames):
    read_jpeg() hands them to the GPU decoder like MjpegAviCapture; width/height from the first frame."""

    def __init__(self, jpegs, fps: float = 30.0):
        self._jpegs = list(jpegs)
        self._i = 0
        self._open = True
        self.fps = float(fps)
        self.w = self.h = 0
        if self._jpegs:
            self.h, self.w = _jpeg_size(self._jpegs[0])
        self._dec = None

    def isOpened(self) -> bool:  # noqa: N802 (cv2 protocol)
        return self._open

    def read_jpeg(self):
        if not self._open or self._i >= len(self._jpegs):
            return False, None
        j = self._jpegs[self._i]
        self._i += 1
        return True, j

    def peek_jpeg(self):
        return self._jpegs[self._i] if self._open and self._i < len(self._jpegs) else None

    def read(self):
        ok, j = self.read_jpeg()
        if not ok:
            return False, None
        if self._dec is None:
            from ._native import MJpegDecoder
            self._dec = MJpegDecoder(self.w, self.h, max_frames=1)
        return True, decode_one(self._dec, j)

    def get(self, prop: int) -> float:
        return {CAP_PROP_FRAME_COUNT: float(len(self._jpegs)), CAP_PROP_FRAME_WIDTH: float(self.w),
                CAP_PROP_FRAME_HEIGHT: float(self.h), CAP_PROP_FPS: self.fps}.get(prop, 0.0)

    def release(self) -> None:
        self._open = False
        if self._dec is not None:
            self._dec.close()
            self._dec = None


def jpeg_layout(data: bytes):
    """(height, width, ((h, v) sampling factors per component)) from a JPEG's SOF marker: frames of one
    GPU decode call must share it."""
    i = 2
    while i + 9 < len(data):
        if data[i] != 0xFF:
            raise ValueError("not a JPEG marker stream")
        m = data[i + 1]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            nc = data[i + 9]
            comps = tuple((data[i + 11 + 3 * c] >> 4, data[i + 11 + 3 * c] & 15) for c in range(nc))
            return (data[i + 5] << 8) | data[i + 6], (data[i + 7] << 8) | data[i + 8], comps
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    raise ValueError("no SOF marker")


def jpeg_gpu_supported(data: bytes) -> bool:
    """Whether the GPU decoder takes this JPEG's layout (fm_jpeg.hip parse_jpeg / setup_geometry):
    SOF0/SOF1 Huffman, 8-bit, one component or three with Cb, Cr at 1x1 and Y at 1x1, 2x1 or 2x2,
    one interleaved scan: the first SOS names every component of the frame, in the frame's order (a
    file whose components come in separate scans is refused by parse_jpeg).  Three components must be
    YCbCr by libjpeg's rule: a JFIF APP0 says so; else an Adobe APP14's transform byte (0: RGB); else
    the ids 'R','G','B' say RGB.  RGB-coded frames go to the host decoder."""
    try:
        i = 2
        if data[:2] != b"\xff\xd8":
            return False
        nc = ids = None
        jfif, adobe = False, None
        while i + 4 <= len(data):
            if data[i] != 0xFF:
                return False
            while i < len(data) and data[i] == 0xFF:
                i += 1
            m = data[i]
            i += 1
            if m == 0xD9 or m == 0x01 or 0xD0 <= m <= 0xD7:
                continue
            ln = (data[i] << 8) | data[i + 1]
            seg = data[i + 2:i + ln]
            if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
                if m not in (0xC0, 0xC1) or seg[0] != 8:
                    return False
                nc = seg[5]
                ids = [seg[6 + 3 * c] for c in range(nc)]
                hv = [(seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15) for c in range(nc)]
                ok = (1 <= hv[0][0] <= 4 and 1 <= hv[0][1] <= 4) if nc == 1 else \
                    (nc == 3 and hv[1] == hv[2] == (1, 1) and hv[0] in ((1, 1), (2, 1), (2, 2)))
                if not ok:
                    return False
            if m == 0xE0 and len(seg) >= 14 and seg[:5] == b"JFIF\0":
                jfif = True
            if m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
            if m == 0xDA:  # the first scan: interleaved over every component of the frame, in its order
                if nc is None or len(seg) < 1 or seg[0] != nc or [seg[1 + 2 * k] for k in range(nc)] != ids:
                    return False
                rgb = adobe == 0 if adobe is not None else ids == [0x52, 0x47, 0x42]
                return not (nc == 3 and not jfif and rgb)
            i += ln
    except IndexError:
        return False
    return False


def decode_one(dec, data: bytes) -> np.ndarray:
    """One frame through a one-frame GPU decoder, or on the host when the GPU decoder refuses this frame's
    layout (FM_ENOTSUP: a later frame of a stream whose first frame it took may be coded differently)."""
    from ._native import FM_ENOTSUP, FMError
    try:
        return dec.decode([data])[0]
    except FMError as e:
        if e.code != FM_ENOTSUP:
            raise
        log.info("JPEG frame not supported by the GPU decoder (%s); decoding it on the host", e)
        return host_decode_jpeg(data)


def host_decode_jpeg(data: bytes) -> np.ndarray:
    """One JPEG -> BGR u8 on the host with libjpeg-turbo: cv2.imdecode when OpenCV exists, else Pillow."""
    if cv2 is not None:
        return cv2.imdecode(np.frombuffer(data, np.uint8), cv2.IMREAD_COLOR)
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im = im.convert("RGB") if im.mode != "RGB" else im
    return np.ascontiguousarray(np.asarray(im)[..., ::-1])


def _jpeg_size(data: bytes):
    """(height, width) from a JPEG's SOF0/SOF1/SOF2 marker."""
    i = 2
    while i + 9 < len(data):
        if data[i] != 0xFF:
            raise ValueError("not a JPEG marker stream")
        m = data[i + 1]
        if m in (0xC0, 0xC1, 0xC2):
            return (data[i + 5] << 8) | data[i + 6], (data[i + 7] << 8) | data[i + 8]
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    raise ValueError("no SOF marker")


class SyntheticCapture(ArrayCapture):
    """The seeded synthetic stream of find_motion_amd.synthetic as a capture (frames made on demand)."""

    def __init__(self, width: int, height: int, n_frames: int, stream: int = 0, seed: int = 1000, start: int = 0):
        from .synthetic import SyntheticVideo

        self.video = SyntheticVideo(width, height, stream, seed=seed)
        self.n_frames, self.start = int(n_frames), int(start)

        class _Lazy:
            def __len__(s):  # noqa: N805
                return self.n_frames

            def __getitem__(s, i):  # noqa: N805
                return self.video.frame(self.start + i)

            @property
            def shape(s):  # noqa: N805
                return (self.n_frames, height, width, 3)

        super().__init__(_Lazy())
        self._first_shape = (height, width, 3)

    def get(self, prop: int) -> float:
        if prop == CAP_PROP_FRAME_COUNT:
            return float(self.n_frames)
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(self._first_shape[1])
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(self._first_shape[0])
        return super().get(prop)


# ---------------------------------------------------------------------------
# YUV frames (what cameras and decoders hand out): the conversion the engine runs on the GPU
# (fm_submit_yuv), vectorised on the host for read() and for frames whose batch is gone

YUV_FOURCCS = {b"NV12": "NV12", b"I420": "I420", b"IYUV": "I420", b"YUY2": "YUY2", b"YUYV": "YUY2", b"UYVY": "UYVY"}
YUV_BITS = {"NV12": 12, "I420": 12, "YUY2": 16, "UYVY": 16}


def yuv_frame_size(w: int, h: int, fmt: str) -> int:
    """Bytes of one tight w x h frame."""
    return w * h * YUV_BITS[fmt] // 8


def yuv_to_bgr(buf, w: int, h: int, fmt: str) -> np.ndarray:
    """One tight YUV frame (bytes-like or uint8 array) -> BGR u8 (h, w, 3): cv2.cvtColor(yuv,
    COLOR_YUV2BGR_{NV12,I420,YUY2,UYVY}) as OpenCV 4.x computes it -- BT.601 limited range in 20-bit fixed
    point, the chroma pair of each 2x1 / 2x2 group replicated (restated from OpenCV's source; the engine's
    GPU conversion is the same arithmetic)."""
    fmt = YUV_FOURCCS.get(fmt, fmt) if isinstance(fmt, bytes) else {"IYUV": "I420", "YUYV": "YUY2"}.get(fmt, fmt)
    if fmt not in YUV_BITS:
        raise ValueError(f"unknown YUV format {fmt!r}")
    if w < 2 or h < 1 or w & 1 or (fmt in ("NV12", "I420") and h & 1):
        raise ValueError(f"{fmt} frames need an even width{' and height' if fmt in ('NV12', 'I420') else ''}")
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, np.uint8).ravel()
    n = yuv_frame_size(w, h, fmt)
    if a.size < n:
        raise ValueError(f"{a.size} bytes for a {w}x{h} {fmt} frame of {n}")
    a = a[:n]
    if fmt == "NV12":
        Y = a[:w * h].reshape(h, w)
        uv = a[w * h:].reshape(h // 2, w // 2, 2)
        U, V = uv[..., 0].repeat(2, 0).repeat(2, 1), uv[..., 1].repeat(2, 0).repeat(2, 1)
    elif fmt == "I420":
        Y = a[:w * h].reshape(h, w)
        q = (w // 2) * (h // 2)
        U = a[w * h:w * h + q].reshape(h // 2, w // 2).repeat(2, 0).repeat(2, 1)
        V = a[w * h + q:].reshape(h // 2, w // 2).repeat(2, 0).repeat(2, 1)
    else:
        p = a.reshape(h, w // 2, 4)
        yi = 0 if fmt == "YUY2" else 1
        Y = p[..., [yi, 2 + yi]].reshape(h, w)
        U, V = p[..., 1 - yi].repeat(2, 1), p[..., 3 - yi].repeat(2, 1)
    y = np.maximum(Y.astype(np.int32) - 16, 0) * 1220542 + (1 << 19)
    uu, vv = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    out = np.empty((h, w, 3), np.uint8)
    out[..., 0] = np.clip((y + 2116026 * uu) >> 20, 0, 255)
    out[..., 1] = np.clip((y - 852492 * vv - 409993 * uu) >> 20, 0, 255)
    out[..., 2] = np.clip((y + 1673527 * vv) >> 20, 0, 255)
    return out


# ---------------------------------------------------------------------------
# uncompressed AVI

def _fourcc(s: str) -> bytes:
    return s.encode("ascii")[:4].ljust(4, b" ")


class RawAviWriter:
    """Uncompressed 24-bit BGR AVI (RIFF, one video stream, idx1 index).

    fourcc ("NV12", "I420", "YUY2", "UYVY"): an uncompressed YUV AVI instead -- write() then takes each frame's
    bytes in that layout (tight, rows top-down) and stores them as they are."""

    def __init__(self, path: str, fps: float, size, fourcc: str | None = None):
        self.path = path
        self.w, self.h = int(size[0]), int(size[1])
        self.fps = max(1, int(round(fps)))
        self.row = (self.w * 3 + 3) & ~3
        self.frame_bytes = self.row * self.h
        self.fourcc = None
        if fourcc is not None:
            self.fourcc = YUV_FOURCCS.get(_fourcc(fourcc))
            if self.fourcc is None:
                raise ValueError(f"RawAviWriter stores BGR or NV12 / I420 / YUY2 / UYVY frames, not {fourcc!r}")
            self.frame_bytes = yuv_frame_size(self.w, self.h, self.fourcc)
        self.n = 0
        self.index = []
        self.f = open(path, "wb")
        self._write_headers()

    def _write_headers(self):
        f = self.f
        f.write(b"RIFF" + struct.pack("<I", 0) + b"AVI ")
        hdrl = bytearray()
        avih = struct.pack("<IIIIIIIIII16x", 1000000 // self.fps, self.frame_bytes * self.fps, 0, 0x10, 0, 0, 1,
                           self.frame_bytes, self.w, self.h)
        hdrl += b"avih" + struct.pack("<I", len(avih)) + avih
        strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", _fourcc(self.fourcc) if self.fourcc else b"DIB ", 0, 0, 0, 0,
                           1, self.fps, 0, 0, self.frame_bytes, 0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        if self.fourcc:
            strf = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, YUV_BITS[self.fourcc], _fourcc(self.fourcc),
                               self.frame_bytes, 0, 0, 0, 0)
        else:
            strf = struct.pack("<IiiHHIIiiII", 40, self.w, self.h, 1, 24, 0, self.frame_bytes, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl += b"LIST" + struct.pack("<I", len(strl)) + strl
        f.write(b"LIST" + struct.pack("<I", len(hdrl) + 4) + b"hdrl" + hdrl)
        self._avih_frames_at = 12 + 8 + 4 + 8 + 16  # RIFF hdr, LIST hdr, 'hdrl', 'avih' hdr, 4 dwords
        self._strh_len_at = 12 + 8 + 4 + 8 + len(avih) + 8 + 4 + 8 + 32
        self._movi_at = f.tell()
        f.write(b"LIST" + struct.pack("<I", 0) + b"movi")

    def isOpened(self) -> bool:  # noqa: N802
        return self.f is not None

    def write(self, frame: np.ndarray) -> None:
        if self.fourcc:
            data = frame.tobytes() if isinstance(frame, np.ndarray) else bytes(frame)
            if len(data) != self.frame_bytes:
                raise ValueError(f"{len(data)} bytes for a {self.w}x{self.h} {self.fourcc} frame of {self.frame_bytes}")
            off = self.f.tell() - (self._movi_at + 8)
            self.f.write(b"00db" + struct.pack("<I", self.frame_bytes) + data + (b"\0" if len(data) & 1 else b""))
            self.index.append(off)
            self.n += 1
            return
        frame = np.asarray(frame, dtype=np.uint8)
        if frame.shape != (self.h, self.w, 3):
            raise ValueError(f"frame shape {frame.shape} != ({self.h}, {self.w}, 3)")
        buf = np.zeros((self.h, self.row), np.uint8)
        buf[:, : self.w * 3] = frame[::-1].reshape(self.h, self.w * 3)  # bottom-up rows
        off = self.f.tell() - (self._movi_at + 8)
        self.f.write(b"00db" + struct.pack("<I", self.frame_bytes))
        self.f.write(buf.tobytes())
        self.index.append(off)
        self.n += 1

    def release(self) -> None:
        if self.f is None:
            return
        f = self.f
        movi_end = f.tell()
        f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
        for off in self.index:
            f.write(b"00db" + struct.pack("<III", 0x10, off, self.frame_bytes))
        end = f.tell()
        f.seek(4)
        f.write(struct.pack("<I", end - 8))
        f.seek(self._movi_at + 4)
        f.write(struct.pack("<I", movi_end - self._movi_at - 8))
        f.seek(self._avih_frames_at)
        f.write(struct.pack("<I", self.n))
        f.seek(self._strh_len_at)
        f.write(struct.pack("<I", self.n))
        f.close()
        self.f = None


class RawAviCapture:
    """Reader for uncompressed 24-bit AVI (what RawAviWriter and OpenCV's 'DIB ' writer produce), and for
    uncompressed YUV AVI: strf compression NV12, I420 / IYUV, YUY2 / YUYV or UYVY (rows top-down, tight).

    A YUV file sets yuv_format ("NV12", "I420", "YUY2", "UYVY"; None for 24-bit files) and gains read_yuv() ->
    (ok, the frame's stored bytes) and peek() (the next frame's bytes, None at the end): BatchFeeder hands the
    bytes to the engine, which converts them on the GPU (fm_submit_yuv).  read() converts on the host
    (yuv_to_bgr) and returns BGR like any capture."""

    def __init__(self, path: str):
        self.path = path
        self._offsets = []
        self.w = self.h = 0
        self.fps = 30.0
        self._i = 0
        self._open = False
        self.yuv_format = None
        try:
            self._parse()
            self._open = self.w > 0 and self.h > 0
        except (OSError, ValueError, struct.error) as e:
            log.error("cannot read %s as uncompressed AVI: %s", path, e)
        if self._open and self.yuv_format:
            self.read_yuv, self.peek = self._read_yuv, self._peek_yuv

    def _parse(self):
        with open(self.path, "rb") as f:
            data = f.read(12)
            if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
                raise ValueError("not a RIFF AVI file")
            size = os.path.getsize(self.path)
            self._walk(f, 12, size, depth=0)
        self._mm = np.memmap(self.path, dtype=np.uint8, mode="r")

    def _walk(self, f, start, end, depth):
        pos = start
        while pos + 8 <= end:
            f.seek(pos)
            ck, ln = struct.unpack("<4sI", f.read(8))
            body = pos + 8
            if ck == b"LIST" or (ck == b"RIFF" and depth == 0):
                # RIFF 'AVIX': the OpenDML continuation of a file past 1 GB, more 'movi' data
                kind = f.read(4)
                if kind in (b"hdrl", b"strl", b"movi", b"rec ", b"AVIX") and depth < 4:
                    self._walk(f, body + 4, min(body + ln, end), depth + 1)
            elif ck == b"avih":
                vals = struct.unpack("<10I", f.read(40))
                if vals[0]:
                    self.fps = 1e6 / vals[0]
            elif ck == b"strf" and not self.w:
                raw = f.read(20)
                bi = struct.unpack("<IiiHHI", raw)
                yuv = YUV_FOURCCS.get(raw[16:20])
                if yuv is not None and bi[4] == YUV_BITS[yuv]:
                    self.w, self.h = bi[1], abs(bi[2])  # (YUV rows are top-down whatever the sign)
                    if self.w & 1 or (yuv in ("NV12", "I420") and self.h & 1):
                        raise ValueError(f"{yuv} AVI of odd size {self.w}x{self.h}")
                    self.yuv_format = yuv
                    self.frame_bytes = yuv_frame_size(self.w, self.h, yuv)
                    pos = body + ln + (ln & 1)
                    continue
                if bi[4] != 24 or bi[5] != 0:
                    raise ValueError(f"only uncompressed 24-bit BGR or NV12 / I420 / YUY2 / UYVY AVI is readable "
                                     f"without OpenCV (bitcount {bi[4]}, compression {bi[5]})")
                self.w, self.h = bi[1], bi[2]
                self._bottom_up = self.h > 0
                self.h = abs(self.h)
                self.row = (self.w * 3 + 3) & ~3
            elif ck[2:] in (b"db", b"dc") and ln > 0:
                self._offsets.append((body, ln))
            pos = body + ln + (ln & 1)

    def isOpened(self) -> bool:  # noqa: N802
        return self._open

    def _peek_yuv(self):
        if not self._open or self._i >= len(self._offsets):
            return None
        off, ln = self._offsets[self._i]
        return self._mm[off: off + self.frame_bytes] if ln >= self.frame_bytes else None

    def _read_yuv(self):
        fr = self._peek_yuv()
        if fr is None:
            return False, None
        self._i += 1
        return True, fr

    def read(self):
        if self.yuv_format:
            ok, fr = self._read_yuv()
            return (True, yuv_to_bgr(fr, self.w, self.h, self.yuv_format)) if ok else (False, None)
        if not self._open or self._i >= len(self._offsets):
            return False, None
        off, ln = self._offsets[self._i]
        self._i += 1
        if ln < self.row * self.h:
            return False, None
        rows = np.asarray(self._mm[off: off + self.row * self.h]).reshape(self.h, self.row)[:, : self.w * 3]
        if self._bottom_up:
            rows = rows[::-1]
        return True, np.ascontiguousarray(rows).reshape(self.h, self.w, 3)

    def get(self, prop: int) -> float:
        return {CAP_PROP_FRAME_COUNT: float(len(self._offsets)), CAP_PROP_FRAME_WIDTH: float(self.w),
                CAP_PROP_FRAME_HEIGHT: float(self.h), CAP_PROP_FPS: self.fps}.get(prop, 0.0)

    def release(self) -> None:
        self._open = False
        self._mm = None


FOURCC_MJPG = b"MJPG"


class MjpegAviCapture(RawAviCapture):
    """MJPEG AVI reader: read_jpeg() -> (ok, JPEG bytes) for the GPU decoder; read() -> (ok, BGR frame).

    gpu_decode (True unless the caller turns it off or the first frame's layout is one the GPU decoder
    does not take, jpeg_gpu_supported): read() decodes on the GPU (a one-frame MJpegDecoder on `device`,
    created on first use) and BatchFeeder hands the compressed frames to fm_submit_jpeg; otherwise
    read() decodes on the host (host_decode_jpeg) and the feeder copies decoded frames."""

    def __init__(self, path: str, device: int = 0, gpu_decode: bool = True):
        self._device = int(device)
        self._dec = None
        super().__init__(path)
        first = self.peek_jpeg()
        self.gpu_decode = bool(gpu_decode) and (first is None or jpeg_gpu_supported(first))
        if gpu_decode and not self.gpu_decode:
            log.info("%s: JPEG layout not supported by the GPU decoder; decoding on the host", path)

    def _walk(self, f, start, end, depth):
        pos = start
        while pos + 8 <= end:
            f.seek(pos)
            ck, ln = struct.unpack("<4sI", f.read(8))
            body = pos + 8
            if ck == b"LIST" or (ck == b"RIFF" and depth == 0):
                # RIFF 'AVIX': the OpenDML continuation of a file past 1 GB, more 'movi' data
                kind = f.read(4)
                if kind in (b"hdrl", b"strl", b"movi", b"rec ", b"AVIX") and depth < 4:
                    self._walk(f, body + 4, min(body + ln, end), depth + 1)
            elif ck == b"avih":
                vals = struct.unpack("<10I", f.read(40))
                if vals[0]:
                    self.fps = 1e6 / vals[0]
            elif ck == b"strf" and not self.w:
                bi = struct.unpack("<IiiHH4s", f.read(20))
                if bi[5] != FOURCC_MJPG:
                    raise ValueError(f"not an MJPEG AVI (compression {bi[5]!r})")
                self.w, self.h = bi[1], abs(bi[2])
            elif ck[2:] == b"dc" and ln > 0:
                self._offsets.append((body, ln))
            pos = body + ln + (ln & 1)

    def read_jpeg(self):
        if not self._open or self._i >= len(self._offsets):
            return False, None
        off, ln = self._offsets[self._i]
        self._i += 1
        return True, bytes(self._mm[off: off + ln])

    def peek_jpeg(self):
        """The next frame's JPEG bytes without consuming it (None at the end)."""
        if not self._open or self._i >= len(self._offsets):
            return None
        off, ln = self._offsets[self._i]
        return bytes(self._mm[off: off + ln])

    def read(self):
        ok, j = self.read_jpeg()
        if not ok:
            return False, None
        if not self.gpu_decode:
            return True, host_decode_jpeg(j)
        if self._dec is None:
            from ._native import MJpegDecoder
            self._dec = MJpegDecoder(self.w, self.h, max_frames=1, device=self._device)
        return True, decode_one(self._dec, j)

    def release(self) -> None:
        super().release()
        if self._dec is not None:
            self._dec.close()
            self._dec = None


class MjpegAviWriter(RawAviWriter):
    """MJPEG AVI writer: frames encoded by Pillow (libjpeg-turbo) at `quality` (default 95, OpenCV's MJPG
    default), one '00dc' chunk per frame.

    encoder (find_motion_amd.MJpegEncoder, or anything with its encode / encode_device): write() encodes on
    the GPU instead, and write_device() takes a frame already in HBM; the bytes are the ones Pillow would
    write for the encoder's settings (which replace quality / jpeg_kw), so the file is the same either way.
    A frame the encoder refuses (FMError) is encoded by Pillow and logged.  device_frames / host_frames /
    fallback_frames count the frames that went each way, encode_calls the calls made to the encoder.

    queue_device() defers a device frame: flush() encodes the queued frames in order, at most
    encoder.max_frames per encoder call, and every other method flushes first, so the file's order is
    always the order of the calls.  A queued address must stay valid until the flush."""

    def __init__(self, path: str, fps: float, size, quality: int = 95, encoder=None, **jpeg_kw):
        self.quality = int(quality)
        self.jpeg_kw = jpeg_kw
        self.encoder = encoder
        self.own_encoder = False  # open_writer made the encoder: release() closes it
        self.device_frames = self.host_frames = self.fallback_frames = self.encode_calls = 0
        self._pending = []  # queue_device: (device address, raw) not yet encoded
        if encoder is not None:
            self.quality = int(getattr(encoder, "quality", quality))
            self.jpeg_kw = dict(jpeg_kw, subsampling=int(getattr(encoder, "subsampling", 2)))
            if getattr(encoder, "restart_interval", 0):
                self.jpeg_kw["restart_marker_blocks"] = int(encoder.restart_interval)
        self.sizes = []
        super().__init__(path, fps, size)

    def _write_headers(self):
        f = self.f
        f.write(b"RIFF" + struct.pack("<I", 0) + b"AVI ")
        mx = self.w * self.h * 3
        hdrl = bytearray()
        avih = struct.pack("<IIIIIIIIII16x", 1000000 // self.fps, mx * self.fps, 0, 0x10, 0, 0, 1, mx, self.w, self.h)
        hdrl += b"avih" + struct.pack("<I", len(avih)) + avih
        strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", FOURCC_MJPG, 0, 0, 0, 0, 1, self.fps, 0, 0, mx,
                           0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, 24, FOURCC_MJPG, mx, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl += b"LIST" + struct.pack("<I", len(strl)) + strl
        f.write(b"LIST" + struct.pack("<I", len(hdrl) + 4) + b"hdrl" + hdrl)
        self._avih_frames_at = 12 + 8 + 4 + 8 + 16
        self._strh_len_at = 12 + 8 + 4 + 8 + len(avih) + 8 + 4 + 8 + 32
        self._movi_at = f.tell()
        f.write(b"LIST" + struct.pack("<I", 0) + b"movi")

    def write_jpeg(self, data: bytes) -> None:
        self.flush()
        self._chunk(data)

    def _chunk(self, data: bytes) -> None:
        off = self.f.tell() - (self._movi_at + 8)
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b""))
        self.index.append(off)
        self.sizes.append(len(data))
        self.n += 1

    def _host_encode(self, frame: np.ndarray) -> bytes:
        import io

        from PIL import Image
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame[..., ::-1])).save(b, "JPEG", quality=self.quality, **self.jpeg_kw)
        return b.getvalue()

    def write(self, frame: np.ndarray) -> None:
        frame = np.asarray(frame, dtype=np.uint8)
        if frame.shape != (self.h, self.w, 3):
            raise ValueError(f"frame shape {frame.shape} != ({self.h}, {self.w}, 3)")
        self.flush()
        if self.encoder is None:
            self._chunk(self._host_encode(frame))
            return
        from ._native import FMError
        try:
            self.encode_calls += 1
            data = self.encoder.encode(frame[None])[0]
            self.host_frames += 1
        except FMError as e:
            log.info("frame refused by the GPU encoder (%s); encoding it on the host", e)
            data = self._host_encode(frame)
            self.fallback_frames += 1
        self._chunk(data)

    def write_device(self, ptr: int, raw=None) -> None:
        """A BGR frame [h][w][3] already in device memory at address ptr, encoded where it lies.  raw: the same
        frame on the host (an array, or a callable that fetches it), used only if the encoder refuses."""
        from ._native import FMError
        if self.encoder is None:
            raise ValueError("write_device needs a writer made with an encoder")
        self.flush()
        self._chunk(self._encode_device_one(ptr, raw))

    def _encode_device_one(self, ptr: int, raw) -> bytes:
        from ._native import FMError
        try:
            self.encode_calls += 1
            data = self.encoder.encode_device([int(ptr)])[0]
            self.device_frames += 1
        except FMError as e:
            if raw is None:
                raise
            log.info("device frame refused by the GPU encoder (%s); encoding it on the host", e)
            data = self._host_encode(np.asarray(raw() if callable(raw) else raw, dtype=np.uint8))
            self.fallback_frames += 1
        return data

    def queue_device(self, ptr: int, raw=None) -> None:
        """write_device, deferred: the frame is encoded and written at the next flush() (which every other
        method starts with), together with the other queued frames.  ptr must stay valid until then."""
        if self.encoder is None:
            raise ValueError("queue_device needs a writer made with an encoder")
        self._pending.append((int(ptr), raw))

    def flush(self) -> None:
        """Encode and write the queued device frames in order, one encoder call per chunk of at most
        encoder.max_frames.  A chunk the encoder refuses goes frame by frame, by write_device's rule."""
        from ._native import FMError
        step = max(1, int(getattr(self.encoder, "max_frames", 1) or 1)) if self.encoder is not None else 1
        while self._pending:
            chunk, self._pending = self._pending[:step], self._pending[step:]
            try:
                self.encode_calls += 1
                datas = self.encoder.encode_device([p for p, _ in chunk])
                self.device_frames += len(chunk)
            except FMError as e:
                if len(chunk) > 1:
                    log.info("%d device frames refused by the GPU encoder (%s); encoding them one by one", len(chunk), e)
                datas = []
                try:
                    for p, raw in chunk:
                        self._chunk(self._encode_device_one(p, raw))
                except FMError:
                    self._pending = []  # (what a failed flush had not written does not stay queued)
                    raise
            for data in datas:
                self._chunk(data)

    def release(self) -> None:
        if self.f is not None and self._pending:
            self.flush()
        if self.own_encoder and self.encoder is not None:
            self.encoder.close()
            self.encoder = None
        if self.f is None:
            return
        f = self.f
        movi_end = f.tell()
        f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
        for off, ln in zip(self.index, self.sizes):
            f.write(b"00dc" + struct.pack("<III", 0x10, off, ln))
        end = f.tell()
        f.seek(4)
        f.write(struct.pack("<I", end - 8))
        f.seek(self._movi_at + 4)
        f.write(struct.pack("<I", movi_end - self._movi_at - 8))
        f.seek(self._avih_frames_at)
        f.write(struct.pack("<I", self.n))
        f.seek(self._strh_len_at)
        f.write(struct.pack("<I", self.n))
        f.close()
        self.f = None


def is_mjpeg_avi(path) -> bool:
    """An AVI whose video stream is MJPG (read by MjpegAviCapture, decoded on the GPU)."""
    try:
        with open(path, "rb") as f:
            head = f.read(4096)
    except (OSError, TypeError):
        return False
    return head[:4] == b"RIFF" and head[8:12] == b"AVI " and FOURCC_MJPG in head


def open_capture(source, device: int = 0, gpu_decode: bool | None = None):
    """cv2.VideoCapture(source) when OpenCV exists (fm.py:413); otherwise the readers above.

    gpu_decode: MJPEG AVI files go to MjpegAviCapture (GPU decode, libjpeg-turbo-exact) when True, or
    when None (the default) and OpenCV is absent.  With OpenCV present and gpu_decode not True the
    reference's own capture is returned, whatever the codec.  gpu_decode=False without OpenCV still
    reads MJPEG AVIs with MjpegAviCapture, decoding on the host.

    `source` may also be an object that already speaks the capture protocol,
    a uint8 array [N][H][W][3], or "synthetic:WxH:N[:stream]".
    """
    if hasattr(source, "read") and hasattr(source, "isOpened"):
        return source
    if isinstance(source, np.ndarray):
        return ArrayCapture(source)
    if isinstance(source, str) and source.startswith("synthetic:"):
        parts = source.split(":")
        w, h = (int(v) for v in parts[1].lower().split("x"))
        return SyntheticCapture(w, h, int(parts[2]), int(parts[3]) if len(parts) > 3 else 0)
    if isinstance(source, str) and source.endswith(".npy"):
        return ArrayCapture(np.load(source, mmap_mode="r", allow_pickle=False))
    if isinstance(source, str) and is_mjpeg_avi(source) and (cv2 is None or gpu_decode):
        cap = MjpegAviCapture(source, device, gpu_decode=gpu_decode is not False)
        if cap.isOpened() and (cap.gpu_decode or cv2 is None):
            return cap  # compressed frames to the GPU decoder (§8(f)-3), or host decode without cv2
        cap.release()  # opted in, but the layout needs the host: the reference's capture
    if cv2 is not None:
        return cv2.VideoCapture(source)
    if isinstance(source, int):
        raise OSError(f"camera {source}: camera capture needs OpenCV, which is not installed")
    return RawAviCapture(str(source))


def open_writer(path: str, codec: str, fps: float, size, jpeg: bool = False, gpu_encode=None, device: int = 0,
                encode_batch: int = 1):
    """cv2.VideoWriter(path, fourcc(codec), fps, size) (fm.py:468-470), else an uncompressed AVI.
    jpeg: the frames come from an MJPEG source -- an 'MJPG' output is then an MjpegAviWriter that
    stores the source's JPEG bytes as they are (write_jpeg), with or without cv2.
    gpu_encode: True (or an encoder object) with codec 'MJPG' -- an MjpegAviWriter whose frames are encoded
    on the GPU (MJpegEncoder on `device`: quality 95, 4:2:0, the bytes Pillow's libjpeg-turbo writes), with
    or without cv2 and for any source but an MJPEG one, whose bytes are still copied.  None / False: as
    without it.  encode_batch: the frames that encoder takes per call (its max_frames; what one flush() of
    queued device frames encodes at once), 1 by default."""
    if jpeg and codec == "MJPG":
        return MjpegAviWriter(path, fps, size)
    if gpu_encode and codec == "MJPG":
        if gpu_encode is True:
            from ._native import MJpegEncoder
            w = MjpegAviWriter(path, fps, size, encoder=MJpegEncoder(int(size[0]), int(size[1]),
                                                                    max_frames=max(1, int(encode_batch)), device=device))
            w.own_encoder = True
            return w
        return MjpegAviWriter(path, fps, size, encoder=gpu_encode)
    if cv2 is not None:
        return cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*codec), fps, size)
    if codec not in ("DIB ", "RGB ", "raw ", None):
        log.debug("OpenCV absent: writing %s as uncompressed AVI instead of codec %s", path, codec)
    return RawAviWriter(path, fps, size)
