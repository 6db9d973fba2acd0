"""ClipBatcher / fami_warp_normalize_batch_u8 on the MI355X: one launch per batch, bit for bit the per-clip kernel
(crop_clip / prepare_clip) and the CPU restatement of cv2.warpAffine + ToTensor + Normalize (oracle/ops.py).  Crops of
(W, H) = (40, 52) are 2080 pixels: eight full workgroups of 256 and a tail of 32."""
import numpy as np
import pytest
import torch

from fami_pose_amd import data as D

pytestmark = pytest.mark.gpu

SIZE = (40, 52)
SRC = [(60, 90), (180, 260), (97, 131)]               # (Hs, Ws) per clip
ROT = [0.0, 31.0, -44.0]
FLIP = [False, True, False]
CENTER = [(50.5, 28.25), (140.5, 80.25), (20.0, 70.0)]          # the crops reach outside the images
SCALE = [(0.45, 0.6), (0.9, 1.2), (0.6, 0.8)]


def _frames(rng, F, Hs, Ws):
    return (rng.rand(F, Hs, Ws, 3) * 255).astype(np.uint8)


def _joints(rng, Hs, Ws):
    joints = np.zeros((17, 3), np.float32)
    joints[:, 0], joints[:, 1] = rng.uniform(0, Ws, 17), rng.uniform(0, Hs, 17)
    vis = np.ones((17, 3), np.float32)
    vis[:, 2] = 0
    vis[rng.randint(0, 17, 3)] = 0
    return joints, vis


def _samples(dev, seed, F, n=3, flips=FLIP):
    """-> (samples for ClipBatcher.prepare with separately allocated frames, the same frames as numpy [F,Hs,Ws,3])"""
    rng = np.random.RandomState(seed)
    samples, host = [], []
    for k in range(n):
        Hs, Ws = SRC[k % 3]
        fr = _frames(rng, F, Hs, Ws)
        joints, vis = _joints(rng, Hs, Ws)
        samples.append({'frames': [torch.from_numpy(fr[f]).to(dev) for f in range(F)], 'joints': joints, 'joints_vis': vis,
                        'center': np.array(CENTER[k % 3]), 'scale': np.array(SCALE[k % 3]), 'rot': ROT[k % 3],
                        'flip': flips[k % 3]})
        host.append(fr)
    return samples, host


def _per_clip(s, size, bgr=False):
    """the parent path on one sample: prepare_clip on the stacked frames -> key, sup, joints [J,2] f32, vis [J] f32, trans"""
    frames = torch.stack(s['frames'])
    key, sup, j, v = D.prepare_clip(frames, s['joints'], s['joints_vis'], s['center'], s['scale'], s['rot'], size,
                                    flip=s['flip'], bgr=bgr)
    c = np.asarray(s['center'], np.float64).copy()
    if s['flip']:
        c[0] = frames.shape[2] - c[0] - 1
    trans = D.dark_get_affine_transform(c, s['scale'], s['rot'], size)
    return key, sup, j[:, :2].astype(np.float32), v[:, 0].astype(np.float32), trans, c


BORDER = torch.tensor([-m / s for m, s in zip(D.MEAN, D.STD)]).view(1, 3, 1, 1)


@pytest.mark.parametrize('bgr', [False, True])
@pytest.mark.parametrize('size', [SIZE, (96, 128)], ids=['40x52', '96x128'])
def test_batched_crop_is_bit_exact_vs_per_clip_kernel_and_oracle(dev, bgr, size):
    from oracle import ops as O
    F = 3
    samples, host = _samples(dev, 21, F)
    b = D.ClipBatcher(3, F, size, bgr=bgr, device=dev)
    kf, sup, _, _, trans, center, scale = b.prepare(samples)
    assert kf.shape == (3, 3, size[1], size[0]) and sup.shape == (3, 3 * (F - 1), size[1], size[0])
    border = False
    for k, s in enumerate(samples):
        key1, sup1, _, _, trans1, c1 = _per_clip(s, size, bgr)
        assert torch.equal(kf[k], key1) and torch.equal(sup[k], sup1), k
        assert np.array_equal(trans[k], trans1) and np.array_equal(center[k], c1)
        assert np.array_equal(trans[k], O.dark_get_affine_transform(c1, s['scale'], s['rot'], size))
        f = k % F                                                 # one frame per clip against the CPU restatement
        img = host[k][f][:, :, ::-1] if bgr else host[k][f]
        want = O.to_tensor_normalize(O.cv2_warp_affine_u8(np.ascontiguousarray(img), trans[k], size, flip=s['flip']),
                                     D.MEAN, D.STD)
        got = (kf[k] if f == 0 else sup[k, 3 * (f - 1):3 * f]).cpu()
        assert torch.equal(got, want), (k, (got - want).abs().max().item())
        border = border or bool((got == BORDER[0]).any())
    assert border                                                 # the zero border occurs
    assert (kf.cpu() == BORDER).any() and np.array_equal(scale, np.array(SCALE))


def test_shared_and_scattered_frames(dev):
    """The evaluation case: four person boxes on one pool of five separately allocated frames, in different orders and
    with overlaps (one clip even names one frame twice)."""
    rng = np.random.RandomState(22)
    Hs, Ws, F = 120, 160, 3
    pool = [torch.from_numpy(_frames(rng, 1, Hs, Ws)[0]).to(dev) for _ in range(5)]
    picks = [(0, 1, 2), (2, 0, 4), (4, 3, 1), (1, 1, 3)]
    samples = []
    for k, pk in enumerate(picks):
        joints, vis = _joints(rng, Hs, Ws)
        samples.append({'frames': [pool[i] for i in pk], 'joints': joints, 'joints_vis': vis,
                        'center': np.array([30.0 + 35 * k, 40.0 + 15 * k]), 'scale': np.array([0.3 + 0.1 * k, 0.4 + 0.13 * k]),
                        'rot': 10.0 * k - 12, 'flip': k % 2 == 1})
    b = D.ClipBatcher(4, F, SIZE, device=dev)
    kf, sup = b.prepare(samples)[:2]
    for k, s in enumerate(samples):
        key1, sup1 = _per_clip(s, SIZE)[:2]
        assert torch.equal(kf[k], key1) and torch.equal(sup[k], sup1), k
    assert not torch.equal(kf[0], kf[1]) and not torch.isnan(kf).any()


def test_short_batch_writes_nothing_else(dev):
    samples, _ = _samples(dev, 23, 3, n=2)
    b = D.ClipBatcher(4, 3, SIZE, device=dev)
    b.kf_x.fill_(float('nan'))
    b.sup_x.fill_(float('nan'))
    b.joints.fill_(float('nan'))
    b.vis.fill_(float('nan'))
    kf, sup, joints, vis = b.prepare(samples)[:4]
    assert kf.shape[0] == sup.shape[0] == joints.shape[0] == vis.shape[0] == 2
    assert kf.data_ptr() == b.kf_x.data_ptr() and joints.data_ptr() == b.joints.data_ptr()
    assert torch.isnan(b.kf_x[2:]).all() and torch.isnan(b.sup_x[2:]).all()
    assert not torch.isnan(b.kf_x[:2]).any() and not torch.isnan(b.sup_x[:2]).any()
    assert not torch.isnan(joints).any() and not torch.isnan(vis).any()
    # F = 1: no supporting frames; the batcher hands the kernel no sup at all ...
    s1, _ = _samples(dev, 24, 1, n=2)
    b1 = D.ClipBatcher(4, 1, SIZE, device=dev)
    b1.kf_x.fill_(float('nan'))
    kf1, sup1 = b1.prepare(s1)[:2]
    assert sup1.shape == (2, 0, SIZE[1], SIZE[0]) and b1.sup_x.numel() == 0
    assert torch.isnan(b1.kf_x[2:]).all() and not torch.isnan(kf1).any()
    for k, s in enumerate(s1):
        assert torch.equal(kf1[k], _per_clip(s, SIZE)[0])
    # ... and the entry point given one (same table, still on the device) leaves it untouched
    from fami_pose_amd._lib import lib
    key2 = torch.full((2, 3, SIZE[1], SIZE[0]), float('nan'), device=dev)
    guard = torch.full((2, 3, SIZE[1], SIZE[0]), float('nan'), device=dev)
    lib().call('fami_warp_normalize_batch_u8', b1._buffers()['dev'].data_ptr(), key2.data_ptr(), guard.data_ptr(), 2, 1,
               SIZE[1], SIZE[0], 0, *D.MEAN, *D.STD, torch.cuda.current_stream(dev).cuda_stream)
    assert torch.equal(key2, kf1) and torch.isnan(guard).all()


def test_rows_beyond_a_short_batch_keep_their_joints(dev):
    """joints / vis rows n.. keep what the batcher last put there (the staging buffer mirrors its device twin)."""
    full, _ = _samples(dev, 25, 2, n=3)
    b = D.ClipBatcher(3, 2, SIZE, device=dev)
    _, _, j0, v0 = b.prepare(full)[:4]
    j0, v0 = j0.clone(), v0.clone()
    short, _ = _samples(dev, 26, 2, n=1)
    b.prepare(short)
    assert torch.equal(b.joints[1:], j0[1:]) and torch.equal(b.vis[1:], v0[1:])
    assert not torch.equal(b.joints[0], j0[0])


def test_joints_visibility_and_transforms_equal_prepare_clip(dev):
    samples, _ = _samples(dev, 27, 2, flips=[True, False, True])
    b = D.ClipBatcher(4, 2, SIZE, device=dev)
    _, _, joints, vis, trans, center, scale = b.prepare(samples)
    assert joints.shape == (3, 17, 2) and vis.shape == (3, 17) and joints.dtype == vis.dtype == torch.float32
    assert joints.is_contiguous() and vis.is_contiguous()
    some_invisible = False
    for k, s in enumerate(samples):
        keep = (s['joints'].copy(), s['joints_vis'].copy(), s['center'].copy())
        _, _, j1, v1, t1, c1 = _per_clip(s, SIZE)
        assert np.array_equal(joints[k].cpu().numpy(), j1) and np.array_equal(vis[k].cpu().numpy(), v1), k
        assert np.array_equal(trans[k], t1) and np.array_equal(center[k], c1)
        assert all(np.array_equal(a, c) for a, c in zip(keep, (s['joints'], s['joints_vis'], s['center'])))
        some_invisible = some_invisible or bool((v1 == 0).any())
    assert some_invisible and trans.shape == (3, 2, 3) and center.shape == scale.shape == (3, 2)


def test_staging_buffer_reuse_back_to_back(dev):
    """Two prepares with different samples and no synchronise between them: the second waits (on the host) only for the
    first one's copy, and overwrites the outputs in stream order."""
    first, _ = _samples(dev, 28, 3)
    second, _ = _samples(dev, 29, 3, flips=[True, False, True])
    want = [[_per_clip(s, SIZE) for s in ss] for ss in (first, second)]
    torch.cuda.synchronize(dev)
    b = D.ClipBatcher(3, 3, SIZE, device=dev)
    out1 = [t.clone() for t in b.prepare(first)[:4]]
    out2 = b.prepare(second)[:4]
    for out, ws in ((out1, want[0]), (out2, want[1])):
        for k, (key1, sup1, j1, v1, _, _) in enumerate(ws):
            assert torch.equal(out[0][k], key1) and torch.equal(out[1][k], sup1), k
            assert np.array_equal(out[2][k].cpu().numpy(), j1) and np.array_equal(out[3][k].cpu().numpy(), v1), k
    assert not torch.equal(out1[0], out2[0]) and not torch.equal(out1[2], out2[2])


def test_straight_into_a_training_step(dev):
    """Trainer(targets_from_joints=True).step(*batcher.prepare(samples)[:4]) against an identically seeded trainer fed by
    the prepare_clip loop: the loss parts are finite and equal bit for bit."""
    import fami_pose_amd as fp
    from fami_pose_amd.train import Trainer
    from oracle import model as om
    S, H, W, B = 2, 128, 96, 2
    rng = np.random.RandomState(30)
    samples = []
    for k in range(B):
        Hs, Ws = SRC[k + 1]
        fr = _frames(rng, 1 + S, Hs, Ws)
        joints, vis = _joints(rng, Hs, Ws)
        samples.append({'frames': [torch.from_numpy(fr[f]).to(dev) for f in range(1 + S)], 'joints': joints,
                        'joints_vis': vis, 'center': np.array([Ws / 2, Hs / 2]), 'scale': np.array([Ws / 260, Hs / 200]),
                        'rot': ROT[k + 1], 'flip': k == 0})
    state = om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), True, S, (H, W)), 5).state_dict()

    def trainer():
        model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
        model.load_state_dict(state)
        return Trainer(model.to(dev).set_deterministic(True), lr=1e-3, use_graph=False, targets_from_joints=True)

    tr_a = trainer()
    batcher = D.ClipBatcher(B, 1 + S, (W, H), device=dev)
    tr_a.step(*batcher.prepare(samples)[:4])
    parts_a = tr_a.loss_parts.clone()
    kf = torch.empty(B, 3, H, W, device=dev)
    sup = torch.empty(B, 3 * S, H, W, device=dev)
    joints, vis = np.zeros((B, 17, 2), np.float32), np.zeros((B, 17), np.float32)
    for k, s in enumerate(samples):
        _, _, j, v = D.prepare_clip(torch.stack(s['frames']), s['joints'], s['joints_vis'], s['center'], s['scale'],
                                    s['rot'], (W, H), flip=s['flip'], out_key=kf[k], out_sup=sup[k])
        joints[k], vis[k] = j[:, :2], v[:, 0]
    tr_b = trainer()
    tr_b.step(kf, sup, torch.from_numpy(joints).to(dev), torch.from_numpy(vis).to(dev))
    assert torch.isfinite(parts_a).all() and (vis > 0).sum() > 8
    assert torch.equal(parts_a, tr_b.loss_parts)
    assert torch.equal(tr_a.flat, tr_b.flat)
