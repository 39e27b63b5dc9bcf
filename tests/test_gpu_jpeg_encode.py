"""Write side on the GPU: MJpegEncoder (fm_mjpeg_enc_*) against Pillow's libjpeg-turbo, byte for byte.

The reference writes motion frames with cv2.VideoWriter, codec 'MJPG' by default (fm.py:303, 447-546).  The GPU
encoder's target is the file Pillow writes for the same pixels and settings -- what videoio.MjpegAviWriter writes
on the host -- so every comparison here is of whole files.  On a mismatch the quantized coefficients are compared
with the numpy restatement (tests/jpeg_encode_ref.py, pinned to Pillow in tests/test_jpeg_encode_host.py) first,
so the failure names the stage: colour / DCT / quantization, header, or entropy coding.

The entropy coder and the stream assembly are pinned on inputs built for them (tests/jpeg_cases.py), whose
properties -- the symbols reached, the byte patterns at the tile seams -- tests/test_jpeg_encode_host.py asserts
from the reference's side: every AC symbol but three, three ZRLs in a block, both signs of every size and DC
category, the quality scaling's clamps and switch, runs of several blocks per lane of k_enc_scan with restart
intervals starting inside them, and FF bytes wherever k_enc_ffcount / k_enc_stuff must decide about them."""
import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_encode_ref as ref
from find_motion_amd import FMError, MJpegDecoder, MJpegEncoder, motion, videoio
from find_motion_amd.synthetic import SyntheticVideo
from jpeg_cases import Image, encode, image, reference_decode

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(Image is None, reason="Pillow not importable")]

SHAPES = [(16, 16), (37, 53), (8, 9), (61, 33), (9, 2), (5, 4), (1, 1), (17, 31)]
SETTINGS = [(95, 2, 0), (30, 2, 0), (95, 0, 0), (50, 1, 0), (100, 2, 0), (80, 2, 3), (70, 1, "row")]
CASES = [(s, c) for s in SHAPES for c in SETTINGS] + [((61, 33), (75, 2, 1))]


def restart_mcus(W, subsampling, restart):
    return -(-W // (8 * ref.SAMPLING[subsampling][0])) if restart == "row" else restart


def pillow(bgr, quality, subsampling, restart=0):
    kw = dict(quality=quality, subsampling=subsampling)
    if restart == "row":
        kw["restart_marker_rows"] = 1
    elif restart:
        kw["restart_marker_blocks"] = restart
    return encode(bgr, **kw)


def assert_equals_pillow(enc, frames, got, want=None):
    """got[i] == Pillow's file for frames[i]; on a mismatch, say which stage differs."""
    assert len(got) == len(frames)
    for i, f in enumerate(frames):
        w = want[i] if want is not None else pillow(f, enc.quality, enc.subsampling, enc.restart_interval)
        if got[i] == w:
            continue
        co, rc = enc.coefficients(i), ref.coefficients(f, enc.quality, enc.subsampling)
        assert co.shape == rc.shape
        bad = np.argwhere(co != rc)
        assert not len(bad), f"frame {i}: {len(bad)} coefficients differ, first at block {bad[0][0]} index {bad[0][1]}"
        n = len(ref.header(f.shape[1], f.shape[0], enc.quality, enc.subsampling, enc.restart_interval))
        assert got[i][:n] == w[:n], f"frame {i}: header differs"
        k = next((k for k in range(min(len(got[i]), len(w))) if got[i][k] != w[k]), min(len(got[i]), len(w)))
        raise AssertionError(f"frame {i}: coefficients equal, entropy-coded bytes differ at {k - n} of the scan "
                             f"({len(got[i])} bytes, Pillow {len(w)})")


@pytest.mark.parametrize("shape,setting", CASES, ids=lambda v: "x".join(str(x) for x in v))
def test_encoder_equals_pillow(shape, setting):
    H, W = shape
    q, s, r = setting
    frames = [image(H, W, kind, seed=sd) for sd, kind in enumerate(["noise", "smooth", "smooth"])]
    enc = MJpegEncoder(W, H, max_frames=4, quality=q, subsampling=s, restart_interval=restart_mcus(W, s, r))
    got = enc.encode(np.stack(frames))
    assert_equals_pillow(enc, frames, got, [pillow(f, q, s, r) for f in frames])
    enc.close()


@pytest.mark.parametrize("name", list(jc.ENTROPY_CASES))
def test_entropy_cases_equal_pillow(name):
    """The symbol sweeps (every 16-bit code of both AC tables, 1 to 3 ZRLs, value at coefficient 63 after them),
    DC differences of every category in both tables, blocks without an EOB, a scan of a few bytes; with a
    restart after every MCU too where the case says so."""
    fn, q, s, restarts = jc.ENTROPY_CASES[name]
    img = fn()
    H, W = img.shape[:2]
    for r in restarts:
        enc = MJpegEncoder(W, H, max_frames=1, quality=q, subsampling=s, restart_interval=r)
        assert_equals_pillow(enc, [img], enc.encode(img))
        enc.close()


# jpeg_set_quality's scaling: 1 and 10 clamp to 255, 23 is the last quality that clamps, 49 / 50 / 51 the switch
QUALITY_SWEEP = [(q, 2) for q in (1, 10, 23, 24, 25, 49, 50, 51, 99)] + [(1, 0)]


@pytest.mark.parametrize("q,s", QUALITY_SWEEP)
def test_quality_sweep_equals_pillow(q, s):
    H, W = 37, 53
    frames = [image(H, W, kind, seed=7) for kind in ("noise", "smooth")]
    enc = MJpegEncoder(W, H, max_frames=2, quality=q, subsampling=s)
    assert_equals_pillow(enc, frames, enc.encode(np.stack(frames)))
    enc.close()


# k_enc_scan gives each of its 256 lanes a run of per = ceil(blocks / 256) consecutive blocks; ib = blocks per
# restart interval.  (H, W, subsampling, restart interval in MCUs):
SCAN_LAYOUT = [
    # 17 x 16 MCUs of 3 blocks = 816 blocks, per = 4.  ib = 3: every run of four holds an interval start inside
    # it, every third run two (at its first and at its last block); ib = 15: a start in four runs of fifteen
    (128, 136, 0, 1), (128, 136, 0, 5),
    # 21 x 7 MCUs of 4 blocks = 588 blocks, per = 3.  ib = 4: intervals longer than a run, a start in three runs
    # of four, at each position of a run in turn; ib = 28: most runs without a start, between runs that have one
    (50, 330, 1, 1), (50, 330, 1, 7),
    # 13 x 8 MCUs of 6 blocks = 624 blocks, per = 3: lanes 208..255 have no blocks.  ib = 6, 12, 78 (a row of 13
    # MCUs) and 618 (103 MCUs: the last interval is one MCU) are multiples of a run: starts at runs' first blocks
    (120, 200, 2, 1), (120, 200, 2, 2), (120, 200, 2, "row"), (120, 200, 2, 103),
]


@pytest.mark.parametrize("H,W,s,r", SCAN_LAYOUT)
def test_scan_layout_with_runs_of_blocks_and_restarts(H, W, s, r):
    frames = [image(H, W, "noise", seed=H + W + k) for k in range(2)]  # noise: block lengths vary
    n = restart_mcus(W, s, r)
    enc = MJpegEncoder(W, H, max_frames=2, quality=90, subsampling=s, restart_interval=n)
    assert -(-enc.blocks // 256) == (4 if s == 0 else 3)
    assert_equals_pillow(enc, frames, enc.encode(np.stack(frames)), [pillow(f, 90, s, r) for f in frames])
    enc.close()


@pytest.mark.parametrize("seed,r,conditions", jc.SEAM_CASES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_seam_frames_equal_pillow(seed, r, conditions):
    """Seven-tile scans in which Pillow's file has (tests/test_jpeg_encode_host.py asserts it) a data FF followed
    by a data D0..D7 with restart markers on, an all-ones byte before an RSTn or the EOI, a data FF on a tile's
    last byte, FF FF across a tile seam."""
    H, W = jc.SEAM_SHAPE
    f = jc.seam_frame(seed)
    enc = MJpegEncoder(W, H, max_frames=1, quality=100, subsampling=0, restart_interval=r)
    assert_equals_pillow(enc, [f], enc.encode(f))
    enc.close()


def _both_orders(enc, frames):
    want = [pillow(f, enc.quality, enc.subsampling, enc.restart_interval) for f in frames]
    assert_equals_pillow(enc, frames, enc.encode(np.stack(frames)), want)
    assert_equals_pillow(enc, frames[::-1], enc.encode(np.stack(frames[::-1])), want[::-1])


@pytest.mark.parametrize("r", [0, 1, 2])
def test_short_stream_between_seven_tile_frames(r):
    """The seam frames of one restart interval in one call, a constant frame (168 bytes of scan: less than 11
    lanes of one tile) after the first; then the same encoder on the reversed order.  Every frame's place in the
    unstuffed buffer, its tiles' numbers and its place in the output depend on the frames before it."""
    H, W = jc.SEAM_SHAPE
    frames = [jc.seam_frame(seed) for seed, ri, _ in jc.SEAM_CASES if ri == r]
    assert len(frames) >= 2
    frames.insert(1, jc.constant(H, W))
    enc = MJpegEncoder(W, H, max_frames=len(frames), quality=100, subsampling=0, restart_interval=r)
    _both_orders(enc, frames)
    enc.close()


@pytest.mark.parametrize("r", [0, 1])
def test_stream_shorter_than_a_lane_between_longer_ones(r):
    """A scan of 14 bytes (a constant 32 x 16 frame, 4:4:4; a few more with restart markers) between scans of
    2.4 KB, the longest this frame size gives: one tile whose only busy lane holds 14 bytes."""
    H, W = jc.SHORT_SHAPE
    frames = [jc.binary_noise(H, W, 0), jc.constant(H, W), jc.binary_noise(H, W, 1), jc.constant(H, W)]
    enc = MJpegEncoder(W, H, max_frames=4, quality=100, subsampling=0, restart_interval=r)
    _both_orders(enc, frames)
    enc.close()


def test_1080p_dummy_block_row_and_buffer_reuse():
    """1080 rows are 67.5 MCU rows at 4:2:0: the last MCU row's lower Y blocks are dummy blocks.  The second call
    has the frames swapped: every offset changes, and nothing of the first call may be left in the buffers."""
    vid = SyntheticVideo(1920, 1080)
    frames = [vid.frame(0), vid.frame(95)]
    want = [pillow(f, 95, 2) for f in frames]
    enc = MJpegEncoder(1920, 1080, max_frames=2)
    assert_equals_pillow(enc, frames, enc.encode(np.stack(frames)), want)
    assert_equals_pillow(enc, frames[::-1], enc.encode(np.stack(frames[::-1])), want[::-1])
    assert_equals_pillow(enc, frames[:1], enc.encode(frames[0]), want[:1])
    assert enc.last_ms() > 0
    enc.close()


def test_wide_frame():
    f = image(19, 3840, "smooth", seed=5)
    enc = MJpegEncoder(3840, 19, max_frames=1)
    assert_equals_pillow(enc, [f], enc.encode(f))
    enc.close()


def test_output_larger_than_the_raw_frame():
    f = image(64, 96, "noise", seed=7)
    enc = MJpegEncoder(96, 64, max_frames=2, quality=100, subsampling=0)
    got = enc.encode(np.stack([f, f]))
    assert len(got[0]) > f.size and b"\xff\x00" in got[0]
    assert_equals_pillow(enc, [f, f], got)
    # a second call with different, shorter content must be exact too
    g = image(64, 96, "smooth", seed=8)
    assert_equals_pillow(enc, [g], enc.encode(g))
    enc.close()


def test_encode_device_equals_host_frames():
    torch = pytest.importorskip("torch")
    H, W = 61, 33
    frames = [image(H, W, kind, seed=sd) for sd, kind in enumerate(["noise", "smooth", "smooth"])]
    enc = MJpegEncoder(W, H, max_frames=4, quality=80, restart_interval=3)
    host = enc.encode(np.stack(frames))
    assert_equals_pillow(enc, frames, host)
    t = torch.from_numpy(np.stack(frames)).to("cuda:0")
    torch.cuda.synchronize()
    assert enc.encode_device(t) == host
    assert enc.encode_device(t.data_ptr(), 3) == host
    parts = [torch.from_numpy(f).to("cuda:0") for f in frames[::-1]]  # three separate allocations
    torch.cuda.synchronize()
    assert enc.encode_device([p.data_ptr() for p in parts]) == host[::-1]
    enc.close()


def test_refusals_leave_the_encoder_usable():
    for kw in (dict(quality=0), dict(subsampling=3)):
        with pytest.raises(FMError):
            MJpegEncoder(16, 16, **kw)
    f = image(16, 16, "smooth")
    enc = MJpegEncoder(16, 16, max_frames=2)
    with pytest.raises(FMError):
        enc.encode(image(16, 24, "smooth"))          # wrong frame size
    with pytest.raises(FMError):
        enc.encode(np.stack([f, f, f]))              # n > max_frames
    with pytest.raises(FMError):
        enc.encode_device([0])                       # a null device address
    with pytest.raises(FMError):
        enc.coefficients(0)                          # nothing encoded yet
    assert_equals_pillow(enc, [f], enc.encode(f))
    enc.close()


@pytest.mark.parametrize("H,W,restart", [(37, 53, 0), (240, 320, "row")])
def test_round_trip_through_the_gpu_decoder(H, W, restart):
    frames = [image(H, W, "smooth", seed=s) for s in range(2)]
    enc = MJpegEncoder(W, H, max_frames=2, quality=90, restart_interval=restart_mcus(W, 2, restart))
    jp = enc.encode(np.stack(frames))
    dec = MJpegDecoder(W, H, max_frames=2)
    got = dec.decode(jp)
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], reference_decode(pillow(f, 90, 2, restart))), i
    dec.close()
    enc.close()


def test_drop_in_writes_the_same_file_as_the_host_writer(tmp_path, monkeypatch):
    """VideoMotion over a raw source with codec 'MJPG': with gpu_encode the written frames are encoded on the GPU
    -- the current frame where the engine holds it in HBM, the frames flushed from the pre-motion cache from
    their host copies -- and the file equals the one MjpegAviWriter writes with Pillow."""
    W, H, n = 320, 240, 40
    real = videoio.open_writer
    out = {}
    for name, flag in (("gpu", True), ("host", None)):
        writers = []
        if flag:
            monkeypatch.setattr(videoio, "open_writer", lambda *a, **kw: writers.append(real(*a, **kw)) or writers[-1])
        else:
            monkeypatch.setattr(videoio, "open_writer", lambda p, c, fps, size, **kw: writers.append(
                videoio.MjpegAviWriter(p, fps, size)) or writers[-1])
        vm = motion.VideoMotion(filename=str(tmp_path / name), capture=videoio.SyntheticCapture(W, H, n, 0),
                                box_size=100, threshold=12, cache_time=0.3, min_time=0.1, batch=4,
                                outdir=str(tmp_path), codec="MJPG", gpu_encode=flag)
        vm.find_motion()
        monkeypatch.setattr(videoio, "open_writer", real)
        out[name] = (vm.written_indices, open(vm.outfile_name, "rb").read(), writers)
    assert out["gpu"][0] and out["gpu"][0] == out["host"][0]
    assert out["gpu"][1] == out["host"][1]
    w = out["gpu"][2][0]
    assert type(w) is videoio.MjpegAviWriter and w.own_encoder
    assert w.device_frames > 0 and w.host_frames > 0 and w.fallback_frames == 0
    assert sum(x.device_frames + x.host_frames for x in out["gpu"][2]) == len(out["gpu"][0])
