"""A box wider than the frame on the GPU (FM_FLAG_AREA_UPSCALE, MotionEngine(area_upscale=True); the detectors'
roi_upscale=True): k_resize_area_up's bytes against the numpy restatement (resize_up_ref.py), then the whole chain,
the detectors' ROI stage and the drop-in against a composed reference -- every frame enlarged by the restatement,
then the oracle at identity on the result (the oracle itself refuses an enlarging resize).

The enlarging rule is restated from knowledge of OpenCV's resize.cpp; parity to cv2 itself is not pinned."""
import functools

import numpy as np
import pytest

import oracle
import pixel_content as pc
import resize_up_ref as ru
from find_motion_amd import FMError, MotionEngine, _native, make_gaussian, rasterize_masks
from find_motion_amd._native import FM_ENOTSUP, PLANE_BLUR, PLANE_DELTA, PLANE_GRAY, PLANE_SMALL, RESIZE_UP
from find_motion_amd.synthetic import batch

pytestmark = pytest.mark.gpu


def _eq(got, ref, msg):
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"{msg}: {len(bad)} mismatches, first {bad[:16].tolist()} "
                             f"got {got[tuple(bad[:8].T)].tolist()} ref {ref[tuple(bad[:8].T)].tolist()}")


def enlarge(frame, box):
    H, W = frame.shape[:2]
    return ru.resize_area_up_u8(frame, box, ru.up_height(H, W, box))


# ---- bytes ------------------------------------------------------------------------------------------------------

def content(W, H, S, T, b):
    """Batch b of [T][S][H][W][3]: seeded noise, the 1-px checkerboard, 2-px column stripes and the dotted white /
    black frames of pixel_content.white, in an order rotated by the stream and the batch, so that 0 / 255
    neighbours meet every coefficient."""
    rng = np.random.default_rng([W, H, b])
    dotted = pc.white(W, H, 1, 6)[:, 0]
    fixed = {"check": np.repeat(pc.checkerboard(H, W)[..., None], 3, -1),
             "cols": np.repeat(pc.stripes(H, W, 1)[..., None], 3, -1), "white_dots": dotted[2], "black_dots": dotted[4]}
    kinds = ["noise", "check", "white_dots", "noise", "cols", "black_dots"]
    out = np.empty((T, S, H, W, 3), np.uint8)
    for t in range(T):
        for s in range(S):
            kind = kinds[(t * S + s + 2 * b) % len(kinds)]
            out[t, s] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if kind == "noise" else fixed[kind]
    return out


BYTES = [  # W, H, box, S, T
    (1, 1, 5, 1, 2),            # the smallest case
    (7, 5, 14, 1, 3),           # exact 2 x: np.repeat
    (64, 48, 128, 2, 3),        # the shape refused without the flag
    (200, 113, 300, 1, 2),      # the ROI's 1.5 x
    (101, 40, 300, 3, 2),       # rows of 900 bytes over frames of 106,200: every alignment over the streams
    (299, 168, 300, 1, 2),      # barely above 1
    (1920, 1080, 1921, 1, 2),   # an identity y axis, 3 w % 4 == 3, two column spans
    (1280, 720, 1920, 1, 2),    # the motivating shape
]


@pytest.mark.parametrize("W,H,box,S,T", BYTES, ids=[f"{c[0]}x{c[1]}-box{c[2]}" for c in BYTES])
def test_enlarged_bytes_equal_the_restatement(W, H, box, S, T):
    """FM_PLANE_SMALL of every frame of every stream over two batches, byte for byte; fm_read_frame still returns
    the source frame."""
    eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=box, ksize=make_gaussian(box, 20), threshold=12,
                       avg=0.1, max_batch=T, area_upscale=True)
    assert eng.resize_kind == RESIZE_UP and eng.work_shape == (ru.up_height(H, W, box), box)
    for b in range(2):
        fr = content(W, H, S, T, b)
        eng.submit(fr)
        eng.wait()
        for t in range(T):
            for s in range(S):
                want = enlarge(fr[t, s], box)
                if box % W == 0:
                    assert np.array_equal(want, np.repeat(np.repeat(fr[t, s], box // W, 0), box // W, 1))
                _eq(eng.plane(PLANE_SMALL, t, s), want, f"small b{b} t{t} s{s}")
        _eq(eng.read_frame(T - 1, S - 1), fr[T - 1, S - 1], f"source frame b{b}")
    eng.close()


def test_enlarged_bytes_from_a_device_buffer_that_ends_with_the_last_frame():
    """Device-resident input whose last frame ends exactly at the end of its allocation (fm_submit on_device = 1):
    the second taps of the last row's last columns are clamped, and nothing is read past them."""
    import torch
    W, H, box, T = 101, 41, 300, 3   # 3 * 101 * 41 * 3 bytes: no multiple of 4
    fr = content(W, H, 1, T, 0)
    dev = torch.from_numpy(fr).to("cuda")
    eng = MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=box, ksize=5, threshold=12, avg=0.1, max_batch=T,
                       area_upscale=True)
    eng.submit_device(dev.data_ptr(), T)
    eng.wait()
    for t in range(T):
        _eq(eng.plane(PLANE_SMALL, t, 0), enlarge(fr[t, 0], box), f"small t{t}")
    eng.close()


# ---- the chain --------------------------------------------------------------------------------------------------

def run_pair(W, H, box, ksize, S=1, T=3, n_batches=2, thresh=12, alpha=0.1, masks=None, keep_planes=False, **kw):
    """tests/test_gpu_parity.py's run_pair with the composed reference: the oracle at identity on the frames
    enlarged by the restatement."""
    eng = MotionEngine(n_streams=S, src_w=W, src_h=H, box_size=box, ksize=ksize, threshold=thresh, avg=alpha,
                       max_batch=T, keep_planes=keep_planes, area_upscale=True, **kw)
    h, w = eng.work_shape
    cfg = oracle.OracleConfig(H=h, W=box, box=box, ksize=ksize, thresh=thresh, alpha=alpha)
    assert (cfg.h, cfg.w) == (h, w) == (ru.up_height(H, W, box), box)
    keeps = [None] * S
    if masks:
        for s in range(S):
            keeps[s] = rasterize_masks(h, w, box / W, masks)
            assert 0 < int((keeps[s] == 0).sum()) < h * w
            eng.set_mask(s, keeps[s])
    orc = [oracle.OracleStream(cfg, keeps[s]) for s in range(S)]
    total = 0
    for b in range(n_batches):
        fr = batch(W, H, S, b * T, T)
        eng.submit(fr)
        eng.wait()
        counts = eng.counts()
        for t in range(T):
            for s in range(S):
                ref = orc[s].step(enlarge(fr[t, s], box))
                tag = f"batch {b} frame {t} stream {s}"
                if keep_planes:
                    _eq(eng.plane(PLANE_GRAY, t, s), ref["gray"], "gray " + tag)
                    _eq(eng.plane(PLANE_BLUR, t, s), ref["blur"], "blur " + tag)
                    _eq(eng.plane(PLANE_DELTA, t, s), ref["delta"], "delta " + tag)
                np.testing.assert_array_equal(eng.mask(t, s), ref["mask"], err_msg="mask " + tag)
                assert counts[t, s] == ref["count"], tag
                cs = eng.contours(t, s)
                assert [c.bbox for c in cs] == ref["boxes"], tag
                assert [c.origin for c in cs] == ref["origins"], tag
                total += ref["count"]
        for s in range(S):
            assert np.array_equal(eng.background(s), orc[s].bg), f"background batch {b} stream {s} not bit-identical"
    assert total > 0, "no contour in any frame: the case shows nothing"
    return eng


CHAIN = [  # W, H, box, k, path, keyword arguments
    (48, 36, 100, 5, "small", {}),
    (200, 113, 300, 5, None, dict(keep_planes=True)),
    (200, 113, 300, 21, None, {}),
    (640, 360, 1088, 51, "wide", dict(T=2)),                      # 17 x 10 tiles
    (64, 48, 128, 5, None, dict(S=3, T=2, masks=[((0, 0), (20, 15)), ((63, 47), (40, 47), (63, 30))])),
    (1280, 720, 1920, 5, None, dict(T=2)),
]


@pytest.mark.parametrize("W,H,box,k,path,kw", CHAIN, ids=[f"{c[0]}x{c[1]}-box{c[2]}-k{c[3]}" for c in CHAIN])
def test_chain_equals_the_oracle_on_enlarged_frames(W, H, box, k, path, kw):
    eng = run_pair(W, H, box, k, **kw)
    if path:
        assert eng.pixel_path == path
    assert eng.pixel_path == _native.plan(src_w=box, src_h=eng.work_shape[0], box_size=box, ksize=k, max_batch=kw.get("T", 3),
                                          n_streams=kw.get("S", 1), keep_planes=kw.get("keep_planes", False))["pixel_path"]
    eng.close()


def test_contour_points_behind_the_enlarging_resize():
    W, H, box, T = 200, 113, 300, 3
    eng = MotionEngine(n_streams=1, src_w=W, src_h=H, box_size=box, ksize=5, threshold=12, avg=0.1, max_batch=T,
                       area_upscale=True, contour_points=True)
    st = oracle.OracleStream(oracle.OracleConfig(H=eng.work_shape[0], W=box, box=box, ksize=5, thresh=12, alpha=0.1))
    fr = batch(W, H, 1, 0, T)
    eng.submit(fr)
    eng.wait()
    seen = 0
    for t in range(T):
        ref = st.step(enlarge(fr[t, 0], box))
        np.testing.assert_array_equal(eng.mask(t, 0), ref["mask"])
        first = oracle.find_contours_ext(ref["mask"], cap=1 << 14)
        cap = max([c["npts"] for c in first], default=0) + 1
        want = oracle.find_contours_ext(ref["mask"], cap=len(first) + 1, with_points=True, pts_cap=cap)
        got = eng.contours(t, 0)
        assert len(got) == len(want) == ref["count"]
        for g, r in zip(got, want):
            assert g.bbox == r["bbox"] and g.origin == r["origin"]
            np.testing.assert_array_equal(g.points[:, 0, :], r["points"])
            assert g.area == r["area"]
        seen += len(want)
    assert seen > 0
    eng.close()


def test_without_the_flag_the_engine_still_refuses():
    with pytest.raises(FMError) as e:
        MotionEngine(n_streams=1, src_w=64, src_h=48, box_size=128, ksize=5, threshold=12, avg=0.1)
    assert e.value.code == FM_ENOTSUP and "INTER_AREA upscaling" in str(e.value)


# ---- the detectors' ROI stage -----------------------------------------------------------------------------------

def _haar_frames(W, H):
    """Three frames of W x H: two of haar_cases.make_image's ROI frames subsampled, one of its painted faces."""
    from haar_cases import draw_faces, make_image
    out = []
    for seed in (0, 1):
        small = make_image(seed, w=300, h=169)
        out.append(np.ascontiguousarray(small[(np.arange(H) * 169) // H][:, (np.arange(W) * 300) // W]))
    out.append(draw_faces(np.empty((H, W, 3), np.uint8), [(W // 3, H // 2, H // 3), (3 * W // 4, H // 2, H // 4)], seed=5))
    return np.stack(out)


@pytest.mark.parametrize("W,H", [(200, 113), (160, 120)])
def test_cascade_on_frames_narrower_than_the_roi(W, H):
    import torch
    from find_motion_amd import CascadeClassifier
    from haar_cases import make_cascade
    from oracle import haar
    cs = make_cascade(1, tight=0.38, depth=2, tilted=True)
    raws = _haar_frames(W, H)
    want = [haar.detect_multiscale(cs, enlarge(f, 300), 1.1, 3) for f in raws]
    assert sum(len(r) for r in want) > 0
    det = CascadeClassifier(cs, roi_upscale=True)
    got = det.detect_frames(raws, 300, 1.1, 3)
    assert [[tuple(r) for r in g.tolist()] for g in got] == want
    ring = torch.zeros((5, H, W, 3), dtype=torch.uint8, device="cuda:0")  # the frame list: out of order, with gaps
    slots = [4, 0, 2]
    for i, k in enumerate(slots):
        ring[k].copy_(torch.from_numpy(raws[i]))
    torch.cuda.synchronize()
    got = det.detect_frame_list([ring[k].data_ptr() for k in slots], H, W, 300, 1.1, 3)
    assert [[tuple(r) for r in g.tolist()] for g in got] == want
    det.close()
    det = CascadeClassifier(cs)
    with pytest.raises(FMError) as e:
        det.detect_frames(raws, 300, 1.1, 3)
    assert e.value.code == FM_ENOTSUP
    det.close()


@functools.lru_cache(maxsize=None)
def _mini():
    import yolo_ref as yr
    _cfg, _weights, layers, params = yr.mini_net()
    return layers, params


def _blob_of_enlarged(frame, net):
    """yolo_ref.blob with the enlarging resize in front."""
    import yolo_ref as yr
    roi = enlarge(frame, 300)
    lin = yr.resize_linear_u8(roi, net, net)
    table = np.array([yr.blob_value(v) for v in range(256)], np.float32)
    return table[lin[:, :, ::-1]].transpose(2, 0, 1).copy(), roi.shape[0]


def test_yolo_on_frames_narrower_than_the_roi():
    import yolo_ref as yr
    from find_motion_amd import YoloDetector
    layers, params = _mini()
    W, H = 200, 113
    frames = yr.make_frames(2, W, H, 11)
    blobs, rh = zip(*[_blob_of_enlarged(f, 64) for f in frames])
    x = np.stack(blobs)
    outs = yr.forward(layers, params, x)
    det = YoloDetector(layers, params, yr.MINI_CLASSES, net_w=64, net_h=64, max_frames=2, roi_upscale=True)
    got = det.detect_frames(frames)
    assert np.array_equal(det.layer_output(-1, 2), x), "the blob of the enlarged frame is not bit-equal"
    for f in range(2):
        bbox, label, conf = yr.detect(yr.decode(layers, outs, 64, 64, 0.2, 0.25, f), 300, rh[0], yr.MINI_CLASSES)
        assert got[f][0] == bbox and got[f][1] == label, f
        assert len(got[f][2]) == len(conf) and np.allclose(got[f][2], conf, rtol=0, atol=1e-4)
    det.close()
    det = YoloDetector(layers, params, yr.MINI_CLASSES, net_w=64, net_h=64, max_frames=2)
    with pytest.raises(FMError) as e:
        det.detect_frames(frames)
    assert e.value.code == FM_ENOTSUP
    det.close()


# ---- the drop-in ------------------------------------------------------------------------------------------------

def test_video_motion_with_a_box_wider_than_the_frames(tmp_path):
    from find_motion_amd import motion, videoio
    from oracle.decision import written_indices
    W, H, box, n = 128, 96, 256, 48
    vid = videoio.SyntheticCapture(W, H, n, 0).video
    frames = [vid.frame(i) for i in range(n)]
    vm = motion.VideoMotion(filename=str(tmp_path / "v"), capture=videoio.ArrayCapture(frames), box_size=box,
                            threshold=12, cache_time=0.3, min_time=0.1, batch=8, outdir=str(tmp_path))
    vm.find_motion()
    k = motion.make_gaussian_size(box, 20)
    st = oracle.OracleStream(oracle.OracleConfig(H=ru.up_height(H, W, box), W=box, box=box, ksize=k))
    counts = [st.step(enlarge(f, box))["count"] for f in frames]
    assert vm.written_indices == written_indices(counts, min_time=0.1, cache_time=0.3)
    assert vm.written_indices
