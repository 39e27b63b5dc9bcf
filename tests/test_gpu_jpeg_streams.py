"""The GPU MJPEG decoder on streams Pillow's default encoder never writes (camera and file MJPEG are the one
input the project does not produce itself): table ids 2 and 3, merged DQT / DHT segments, 16-bit quantization
tables, three quantization tables, other component ids, Adobe and JFIF metadata, APPn / COM payloads that
hold marker bytes, bytes after EOI, no EOI, a gray frame's sampling byte, and the entropy coder's extremes
(with Pillow's files of the inputs the GPU encoder's entropy coder is pinned on: its symbol sweeps and seam frames).

Every comparison is np.array_equal against Pillow's libjpeg-turbo decode of the same bytes; where a patch
keeps the stream's meaning, Pillow's decode of the patched bytes must equal its decode of the unpatched ones,
so a broken helper fails as a helper.  Each case runs at the decoder's default chunking and at 64-bit chunks
without speculation (every chunk boundary a fix-up).  RGB-coded streams (libjpeg's colour-space rule), a scan
out of the frame's component order and CMYK are refused, and the decoder goes on decoding."""
import numpy as np
import pytest

from find_motion_amd import FMError, MJpegDecoder
from find_motion_amd._native import FM_EINVAL, FM_ENOTSUP
from jpeg_cases import (ENTROPY_CASES, REFUSED, RGB_REFUSED, SEAM_CASES, SEAM_SHAPE, STREAMS, SUBSAMPLINGS, Image, as_jfif,
                        busy_noise, checkerboard, constant, encode, image, luma_dc_differences, reference_decode,
                        restart_interval_lengths, seam_frame, stream_reference)
from oracle import jpeg

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(Image is None, reason="Pillow not importable")]

SHAPES = [(37, 53), (16, 16)]
WIDE = (19, 3840)  # bands narrower than a block row: k_jpeg_idct dequantizes every block, not the colour kernel
CHUNKINGS = [dict(), dict(chunk_bits=64, spec_bits=0)]


def _decode_alone(data, H, W, want):
    """One stream alone in its own call, on a fresh decoder per chunking."""
    for kw in CHUNKINGS:
        dec = MJpegDecoder(W, H, max_frames=1, **kw)
        got = dec.decode([data])
        dec.close()
        assert got.shape == (1, H, W, 3)
        assert np.array_equal(got[0], want), kw


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_variant(name, H, W):
    data, base = STREAMS[name](H, W)
    want = stream_reference(name, data)
    if base is not None:
        assert data != base and np.array_equal(want, reference_decode(base))
    _decode_alone(data, H, W, want)


@pytest.mark.parametrize("name", ["dqt16_sof1", "merged_dqt16"])
def test_16_bit_tables_on_wide_frames(name):
    """3840 wide: quantizers past 255 through k_jpeg_idct's dequantization instead of the fused one."""
    H, W = WIDE
    data, base = STREAMS[name](H, W)
    assert int(jpeg.parse(data)["qt"][1].max()) == 1000
    want = reference_decode(data)
    if base is not None:
        assert np.array_equal(want, reference_decode(base))
    _decode_alone(data, H, W, want)


MIXED = ["plain", "huff_ids_2_3", "merged_dht", "dqt16_sof1", "three_qtables", "app2_com_markers", "trailing_bytes"]


@pytest.mark.parametrize("H,W", SHAPES)
def test_mixed_call_on_one_decoder(H, W):
    """Frames of one geometry whose table sets differ, in one call: runs split where the Huffman slots change,
    quantization tables per frame.  In that order and reversed, each call twice on the same decoder (the
    coefficient buffer must come back zeroed).  Every frame has its own image, so a frame taken for another
    shows."""
    frames = []
    for s, name in enumerate(MIXED):
        frames.append(encode(image(H, W, "smooth", seed=10 + s), quality=85) if name == "plain" else
                      STREAMS[name](H, W, 10 + s)[0])
    want = [reference_decode(f) for f in frames]
    assert all(not np.array_equal(want[i], want[j]) for i in range(len(want)) for j in range(i))
    for kw in CHUNKINGS:
        dec = MJpegDecoder(W, H, max_frames=len(frames), **kw)
        for order in (slice(None), slice(None, None, -1)):
            for _ in range(2):
                got = dec.decode(frames[order])
                for i, w in enumerate(want[order]):
                    assert np.array_equal(got[i], w), (kw, MIXED[order][i])
        dec.close()


def _extreme_shapes():
    return [pytest.param(H, W, id=f"{H}x{W}") for H, W in SHAPES + [WIDE]]


@pytest.mark.parametrize("H,W", _extreme_shapes())
@pytest.mark.parametrize("sub,ss", SUBSAMPLINGS)
def test_dc_difference_of_category_11(sub, ss, H, W):
    """Black and white 8 x 8 blocks at quality 100: a luma DC difference of 2040, a 9-bit code and 11 extra
    bits, past the 10-bit fast table."""
    data = encode(checkerboard(H, W), quality=100, subsampling=ss)
    j = jpeg.parse(data)
    assert max(abs(v) for v in luma_dc_differences(j, jpeg.decode_coefficients(j))) == 2040
    _decode_alone(data, H, W, reference_decode(data))


@pytest.mark.parametrize("H,W", _extreme_shapes())
@pytest.mark.parametrize("sub,ss", SUBSAMPLINGS)
def test_blocks_without_an_eob(sub, ss, H, W):
    """Noise at quality 100: coefficient 63 is non-zero in every luma block of the image (the blocks that only
    pad the last MCU are empty by the encoder's construction), so no such block ends in an EOB."""
    data = encode(busy_noise(H, W), quality=100, subsampling=ss)
    luma = jpeg.decode_coefficients(jpeg.parse(data))[0]
    assert np.all(luma[:-(-H // 8), :-(-W // 8), 63] != 0)
    _decode_alone(data, H, W, reference_decode(data))


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("sub,ss", SUBSAMPLINGS)
def test_restart_intervals_of_a_few_bytes(sub, ss, H, W):
    """A constant image with a restart after every MCU: intervals of 2 to 4 bytes, many inside one chunk."""
    data = encode(constant(H, W), quality=75, subsampling=ss, restart_marker_blocks=1)
    lens = restart_interval_lengths(jpeg.parse(data))
    assert len(lens) == -(-H // (16 if ss == 2 else 8)) * -(-W // (8 if ss == 0 else 16)) and min(lens) <= 4
    _decode_alone(data, H, W, reference_decode(data))


SWEEPS = [(n, 0) for n in ENTROPY_CASES if n.startswith("sweep_")] + [("sweep_luma_q100", 1), ("sweep_chroma_q50", 1)]


@pytest.mark.parametrize("name,restart", SWEEPS)
def test_symbol_sweeps(name, restart):
    """Pillow's files of the encoder's symbol sweeps (tests/test_jpeg_encode_host.py counts what they reach: all
    but three of the 2 x 162 AC symbols, so every 16-bit code, with up to 10 extra bits, on the path past the
    10-bit lookup table; three ZRLs in a block; a value at coefficient 63 after them)."""
    fn, q, ss, _ = ENTROPY_CASES[name]
    img = fn()
    data = encode(img, quality=q, subsampling=ss, **(dict(restart_marker_blocks=restart) if restart else {}))
    _decode_alone(data, img.shape[0], img.shape[1], reference_decode(data))


@pytest.mark.parametrize("seed,restart,conditions", SEAM_CASES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_seam_frames(seed, restart, conditions):
    """The encoder's seam frames, read: 25 KB scans with a data FF before a data D0..D7 among restart markers,
    all-ones bytes before RSTn and EOI."""
    H, W = SEAM_SHAPE
    data = encode(seam_frame(seed), quality=100, subsampling=0, **(dict(restart_marker_blocks=restart) if restart else {}))
    _decode_alone(data, H, W, reference_decode(data))


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_leave_the_decoder_usable(name, H, W):
    """RGB-coded planes and four components: FM_ENOTSUP, the status on which decode_one and the feeder decode
    on the host.  A scan out of the frame's order: refused as libjpeg refuses it.  Before and after, the same
    decoder decodes valid frames bit-exactly."""
    bad = REFUSED[name](H, W)
    good = [encode(image(H, W, "smooth", seed=s), quality=85, subsampling=0) for s in (20, 21)]
    for kw in CHUNKINGS:
        dec = MJpegDecoder(W, H, max_frames=2, **kw)
        assert np.array_equal(dec.decode([good[0]])[0], reference_decode(good[0]))
        for frames in ([bad], [good[0], bad]):
            with pytest.raises(FMError) as e:
                dec.decode(frames)
            assert e.value.code == (FM_EINVAL if name == "sos_ids_swapped" else FM_ENOTSUP)
        got = dec.decode(good[::-1])
        assert np.array_equal(got[0], reference_decode(good[1])) and np.array_equal(got[1], reference_decode(good[0]))
        dec.close()
        dec = MJpegDecoder(W, H, max_frames=1, **kw)  # refused as a decoder's first frame, before it has a geometry
        with pytest.raises(FMError):
            dec.decode([bad])
        assert np.array_equal(dec.decode([good[1]])[0], reference_decode(good[1]))
        dec.close()
    if name in RGB_REFUSED:  # what the GPU would have returned: libjpeg does not take these planes as YCbCr
        assert not np.array_equal(reference_decode(bad), reference_decode(as_jfif(bad)))


@pytest.mark.parametrize("name", RGB_REFUSED)
def test_decode_one_hands_rgb_streams_to_the_host(name):
    """FM_ENOTSUP is the status on which videoio.decode_one decodes on the host: the frame comes out as
    libjpeg returns it, and the decoder takes the next frame."""
    from find_motion_amd import videoio
    H, W = 37, 53
    bad, good = REFUSED[name](H, W), encode(image(H, W, "smooth", seed=22), quality=85)
    dec = MJpegDecoder(W, H, max_frames=1)
    assert np.array_equal(videoio.decode_one(dec, bad), reference_decode(bad))
    assert np.array_equal(videoio.decode_one(dec, good), reference_decode(good))
    dec.close()
