"""Per-launch times of the f32 split-product band kernel (conv_t4.hip) with the persistent kernel off, as tools/bench_t5.py's
"band" column, under a list of tune settings: the register form (102040) against the weight-DMA form (102041), alone and with
the band-filling (102001) / narrow-block (102031) switches that weight staging decided.  Rows: the two low-resolution branch
shapes, the head's 4-frame 96x72 convolution, the dilated 48 -> 324 predictor.  Median of 5 timings of 200 launches.  GPU box.
usage: python tools/bench_band_wdma.py [name=code+code ...]      (no argument: the library's default route only)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fami_pose_amd._lib import lib
L = lib(); dev = torch.device('cuda:0'); s = torch.cuda.current_stream(dev); st = s.cuda_stream
def timeit(fn, reps=200, n=5):
    for _ in range(10): fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps): fn()
        e1.record(s); e1.synchronize()
        ts.append(e0.elapsed_time(e1) / reps * 1e3)
    return sorted(ts)[n // 2]
p = lambda t: None if t is None else t.data_ptr()
settings = [('default', [])] + [(a.split('=')[0], [int(c) for c in a.split('=')[1].split('+')]) for a in sys.argv[1:]]
shapes = [(20, 24, 18, 192, 192, 1), (20, 12, 9, 384, 384, 1), (4, 96, 72, 48, 48, 1), (4, 96, 72, 48, 324, 3)]
for (N, H, W, Ci, Co, dil) in shapes:
    x = torch.randn(N, H, W, Ci, device=dev); y = torch.empty(N, H, W, Co, device=dev)
    dy = torch.randn(N, H, W, Co, device=dev); dx = torch.empty_like(x)
    w = torch.randn(Co, Ci, 3, 3, device=dev) * 0.05
    geo = (N, H, W, Ci, Co, 3, 3, 1, dil, dil)
    wp0 = torch.empty(L.cdll.fami_packed_weight_elems(Co, Ci, 3, 3, 0), device=dev); wp1 = torch.empty(L.cdll.fami_packed_weight_elems(Co, Ci, 3, 3, 1), device=dev)
    L.call('fami_pack_conv_weight_f32', p(w), p(wp0), Co, Ci, 3, 3, 0, st); L.call('fami_pack_conv_weight_f32', p(w), p(wp1), Co, Ci, 3, 3, 1, st)
    fwd = lambda: L.call('fami_conv2d_fwd_f32', p(x), p(wp0), None, None, p(y), *geo, 0, 0, st)
    bwd = lambda: L.call('fami_conv2d_dgrad_f32', p(dy), p(wp1), None, p(dx), *geo, 0, st)
    res, ref = [], None
    for name, codes in settings:
        L.cdll.fami_conv_tune_lds(-1); L.cdll.fami_conv_tune_lds(7000)
        for c in codes: L.cdll.fami_conv_tune_lds(c)
        res.append((name, timeit(fwd), timeit(bwd)))
        torch.cuda.synchronize()
        ref = y.clone() if ref is None else ref
        assert torch.equal(ref, y), (name, 'forward differs from the first setting')
    L.cdll.fami_conv_tune_lds(-1)
    gf = 2.0 * N * H * W * Ci * Co * 9 / 1e9
    print('f32 N%-2d %3dx%-3d %3d->%-3d dil %d %.2f GFLOP fwd/dgrad us | ' % (N, H, W, Ci, Co, dil, gf) + ' | '.join('%s %.1f/%.1f' % r for r in res), flush=True)
