"""numpy / torch restatements of the three supervision options -- the yardsticks of tests/test_loss_options_host.py,
tests/test_loss_options_gpu.py and tests/test_train_gpu_loss_options.py.

    1. `gauss_targets`: generate_heatmaps (datasets/process/heatmaps_process.py:146-203) for a batch, with the per-joint
       weights of :200-201 and the two encodings.
         quantised: the reference's own arithmetic, a float32 19x19 patch exp(-((x - 9)^2 + (y - 9)^2) / (2 sigma^2))
                    pasted at the rounded centre (mx, my) = int(joint / stride + 0.5), truncating toward zero;
         subpixel:  float64, exp(-((x - cx)^2 + (y - cy)^2) / (2 sigma^2)) with (cx, cy) = joint / stride, on the SAME
                    window [mx - 3 sigma, mx + 3 sigma] x [my - 3 sigma, my + 3 sigma] clipped to the map.
       The weight is the visibility, 0 where the patch lies wholly outside the map, times joint_weights[j] (a float32
       product, as numpy.multiply on two float32 arrays); the map is drawn where the UNMULTIPLIED weight is > 0.5.
    2. `ohkm_ref`: per sample the k joints with the largest row loss mean_p (w (pred - gt))^2 -- larger first, equal
       values by lower joint index, NaN above every number -- value (1/B) sum_b (1/k) sum_selected, float64, with the
       analytic gradient 2 w^2 (pred - gt) / (B k L) on the selected joints and 0 elsewhere.
    3. `hrnet_ohkm_torch`: a literal torch transcription of the HRNet family's JointsOHKMMSELoss (MSELoss(reduction=
       'none') per joint, mean over pixels, torch.topk per sample, sum / topk, mean over samples) with its factor 0.5
       removed -- what 2 is checked against, in value and in autograd gradient.
`dark_round_trip_joints` draws the joints of the DARK round trip: real-valued centres at least `margin` heatmap pixels
from every border."""
import numpy as np
import torch


def gauss_targets(joints, vis, sigma, image_size, heatmap_size, encoding='quantised', joint_weights=None):
    """joints [B,J,2|3] pixels, vis [B,J]; image_size / heatmap_size (w, h) -> target [B,J,Hh,Wh] (float32 for
    'quantised', float64 for 'subpixel'), weight [B,J,1] float32."""
    assert encoding in ('quantised', 'subpixel')
    joints = np.asarray(joints, np.float32)
    vis = np.asarray(vis, np.float32)
    B, J = joints.shape[:2]
    Wh, Hh = int(heatmap_size[0]), int(heatmap_size[1])
    stride = np.asarray(image_size, np.float64) / np.asarray(heatmap_size)
    r = sigma * 3
    ax = np.arange(0, 2 * r + 1, 1, np.float32)
    patch = np.exp(-((ax[None, :] - r) ** 2 + (ax[:, None] - r) ** 2) / (2 * sigma ** 2))
    assert patch.dtype == np.float32
    sub = encoding == 'subpixel'
    target = np.zeros((B, J, Hh, Wh), np.float64 if sub else np.float32)
    weight = vis.reshape(B, J, 1).copy()
    for b in range(B):
        for j in range(J):
            cx, cy = float(joints[b, j, 0]) / stride[0], float(joints[b, j, 1]) / stride[1]
            mx, my = int(cx + 0.5), int(cy + 0.5)
            x0, y0, x1, y1 = mx - r, my - r, mx + r + 1, my + r + 1
            if x0 >= Wh or y0 >= Hh or x1 < 0 or y1 < 0:
                weight[b, j] = 0
                continue
            if not weight[b, j, 0] > 0.5:
                continue
            xs, ys = slice(max(0, x0), min(x1, Wh)), slice(max(0, y0), min(y1, Hh))
            if sub:
                xx = np.arange(xs.start, max(xs.stop, xs.start), dtype=np.float64)[None, :]
                yy = np.arange(ys.start, max(ys.stop, ys.start), dtype=np.float64)[:, None]
                target[b, j, ys, xs] = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma ** 2))
            else:
                target[b, j, ys, xs] = patch[max(0, -y0):min(y1, Hh) - y0, max(0, -x0):min(x1, Wh) - x0]
    if joint_weights is not None:
        jw = np.asarray(joint_weights, np.float32).reshape(1, J, 1)
        weight = np.multiply(weight, jw)
    assert weight.dtype == np.float32
    return target, weight


def ohkm_order(rows):
    """[J] row losses -> the joint indices in ranking order: NaN first, then larger first, equal values by lower index."""
    rows = np.asarray(rows, np.float64)
    return sorted(range(len(rows)), key=lambda j: (0, 0.0, j) if np.isnan(rows[j]) else (1, -rows[j], j))


def ohkm_select(rowsums, k):
    """[B,J] row sums (or losses) -> bool [B,J]: the k first of ohkm_order per sample."""
    rowsums = np.asarray(rowsums)
    sel = np.zeros(rowsums.shape, bool)
    for b in range(rowsums.shape[0]):
        sel[b, ohkm_order(rowsums[b])[:k]] = True
    return sel


def ohkm_ref(pred, gt, w, k):
    """pred, gt [B,J,...], w [B,J] or None -> (value, selection bool [B,J], gradient like pred), float64."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    B, J = pred.shape[:2]
    L = int(np.prod(pred.shape[2:]))
    wv = np.ones((B, J)) if w is None else np.asarray(w, np.float64).reshape(B, J)
    d = (pred - gt).reshape(B, J, L) * wv[:, :, None]
    rows = (d * d).mean(2)
    sel = ohkm_select(rows, k)
    value = sum(rows[b][sel[b]].sum() / k for b in range(B)) / B
    grad = 2.0 * d * wv[:, :, None] * sel[:, :, None] / (B * k * L)
    return value, sel, grad.reshape(pred.shape)


def hrnet_ohkm_torch(output, target, target_weight, topk, use_target_weight=True):
    """JointsOHKMMSELoss.forward of the HRNet family without its factor 0.5 (torch, differentiable in `output`)."""
    criterion = torch.nn.MSELoss(reduction='none')
    batch_size, num_joints = output.size(0), output.size(1)
    heatmaps_pred = output.reshape((batch_size, num_joints, -1)).split(1, 1)
    heatmaps_gt = target.reshape((batch_size, num_joints, -1)).split(1, 1)
    loss = []
    for idx in range(num_joints):
        heatmap_pred = heatmaps_pred[idx].squeeze(1)
        heatmap_gt = heatmaps_gt[idx].squeeze(1)
        if use_target_weight:
            loss.append(criterion(heatmap_pred.mul(target_weight[:, idx]), heatmap_gt.mul(target_weight[:, idx])))
        else:
            loss.append(criterion(heatmap_pred, heatmap_gt))
    loss = torch.cat([l.mean(dim=1).unsqueeze(dim=1) for l in loss], dim=1)
    ohkm_loss = 0.
    for i in range(batch_size):
        sub_loss = loss[i]
        _, topk_idx = torch.topk(sub_loss, k=topk, dim=0, sorted=False)
        ohkm_loss = ohkm_loss + torch.sum(torch.gather(sub_loss, 0, topk_idx)) / topk
    return ohkm_loss / batch_size


def dark_round_trip_joints(seed, B, J, H, W, stride=4, margin=10):
    """-> joints [B,J,2] float32 image pixels whose heatmap positions joint / stride lie in [margin, W - 1 - margin] x
    [margin, H - 1 - margin], and those positions [B,J,2] in float64 (of the ROUNDED float32 joints)."""
    rng = np.random.RandomState(seed)
    c = np.stack([rng.uniform(margin, W - 1 - margin, (B, J)), rng.uniform(margin, H - 1 - margin, (B, J))], -1)
    joints = (c * stride).astype(np.float32)
    return joints, joints.astype(np.float64) / stride
