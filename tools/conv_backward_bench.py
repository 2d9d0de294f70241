"""Convolution backward (dx + dw + db in one srcnn_conv2d_backward call) against torch's own fp32 convolution backward.

    python tools/conv_backward_bench.py [--out profiles/conv_backward_bench.txt] [--reps 50]
    python tools/conv_backward_bench.py --precision f16x3 --out profiles/conv_backward_f16x3_bench.txt

Shapes: the trainable trunk and head at B = 1, one 600 x 1987 image (pyramid maps 150x497, 75x249, 38x125, 19x63) -- the (M, N, K)
of the per-layer table (stereo_rcnn_amd/layer_table.py) for a representative bottleneck of layer2 / layer3 / layer4, an FPN lateral
and a smooth conv, RPN_Conv and the 24-channel RPN head on P2, RCNN_top and the stacked linear heads at 512 rois
(cfg.TRAIN.BATCH_SIZE).  layer0 / layer1 are frozen in the reference and not listed.
  * hip   : srcnn_conv2d_backward (mask / bias pass, weight re-layout, dgrad, wgrad, split-K reduction -- everything the call
            issues, the re-layout included: weights change every step), heuristic tiles and splits, ReLU mask on;
  * torch : aten.convolution_backward (dx, dw, db) on the same values in NCHW float32 plus the ReLU's threshold_backward, i.e.
            what torch.autograd runs for relu(conv(x)) on this device;
  * fwd   : the exact-fp32 forward (srcnn_conv2d, precision 0, heuristic plan) of the same layer, the second yardstick.
--precision f16x3 adds a column: srcnn_conv2d_backward_f16x3 (the 3 x f16 split; its clear / max / split passes included) on the
same layers, alternating with the fp32 backward inside every round -- the yardstick is that fp32 column -- and f16x3 / hip.
FLOPs: 2 M N K for the forward, twice that for the backward (dgrad + wgrad), whatever zeros a stride multiplies.
One process, 10 untimed runs of each first; hip and torch ALTERNATE; every run is timed with device events; medians of --reps.
Runner and timer: tools/benchlib.py."""
import benchlib

# name, B, H, W, Cin, Cout, k, stride, pad
LAYERS = [
    ('layer2.conv2 3x3', 1, 75, 249, 128, 128, 3, 1, 1),
    ('layer2.conv3 1x1', 1, 75, 249, 128, 512, 1, 1, 0),
    ('layer2.downsample 1x1/2', 1, 150, 497, 256, 512, 1, 2, 0),
    ('layer3.conv1 1x1', 1, 38, 125, 1024, 256, 1, 1, 0),
    ('layer3.conv2 3x3', 1, 38, 125, 256, 256, 3, 1, 1),
    ('layer3.conv3 1x1', 1, 38, 125, 256, 1024, 1, 1, 0),
    ('layer3.downsample 1x1/2', 1, 75, 249, 512, 1024, 1, 2, 0),
    ('layer4.conv2 3x3', 1, 19, 63, 512, 512, 3, 1, 1),
    ('layer4.conv3 1x1', 1, 19, 63, 512, 2048, 1, 1, 0),
    ('fpn.lateral C2 1x1', 1, 150, 497, 256, 256, 1, 1, 0),
    ('fpn.smooth P2 3x3', 1, 150, 497, 256, 256, 3, 1, 1),
    ('RPN_Conv P2 3x3', 1, 150, 497, 256, 512, 3, 1, 1),
    ('RPN head P2 1x1 (24)', 1, 150, 497, 512, 24, 1, 1, 0),
    ('RCNN_top 7x7/7, 512 rois', 512, 7, 7, 512, 2048, 7, 7, 0),
    ('RCNN_top 1x1, 512 rois', 512, 1, 1, 2048, 2048, 1, 1, 0),
    ('linear heads (24), 512 rois', 512, 1, 1, 2048, 24, 1, 1, 0),
]


def child(reps, precision='f32'):
    import torch
    from stereo_rcnn_amd import engine
    dev = benchlib.device()
    aten = torch.ops.aten
    f16 = precision == 'f16x3'
    print('%-30s %9s %6s %7s | %9s %7s | %9s %7s | %9s %7s' % ('layer', 'M', 'N', 'K', 'hip us', 'TF/s', 'torch us', 'TF/s', 'hip/torch', 'fwd TF/s')
          + (' | %9s %7s %9s' % ('f16x3 us', 'TF/s', 'f16x3/hip') if f16 else ''))
    for name, B, H, W, cin, cout, k, s, p in LAYERS:
        gen = torch.Generator().manual_seed(1)
        OH, OW = engine.conv_out_hw(H, W, k, k, s, p)
        x = torch.randn(B, H, W, cin, generator=gen).to(dev)
        w = (torch.randn(cout, k, k, cin, generator=gen) / float(k * k * cin) ** 0.5).to(dev)
        dy = torch.randn(B, OH, OW, cout, generator=gen).to(dev)
        cw = engine.ConvW(w, torch.zeros(cout, device=dev), k, k, s, p, True)
        y = torch.empty(B, OH, OW, cout, device=dev)
        out = {'dx': torch.empty(B, H, W, cin, device=dev), 'dw': torch.empty_like(w), 'db': torch.empty(cout, device=dev)}
        xn, wn = x.permute(0, 3, 1, 2).contiguous(), w.permute(0, 3, 1, 2).contiguous()
        yn, dyn = None, dy.permute(0, 3, 1, 2).contiguous()

        def fwd():
            engine.conv2d(cw, x, B, H, W, y, OH, OW, precision='f32', plan=(0, 0, 0, 0, 0))

        def hip():
            engine.conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, out=out)

        out3 = {k_: torch.empty_like(v) for k_, v in out.items()}

        def hip3():
            engine.conv2d_backward(cw, x, B, H, W, y, dy, OH, OW, out=out3, precision='f16x3')

        def eager():
            g = aten.threshold_backward(dyn, yn, 0)
            return aten.convolution_backward(g, xn, wn, [cout], [s, s], [p, p], [1, 1], False, [0, 0], 1, [True, True, True])

        fwd()
        yn = y.permute(0, 3, 1, 2).contiguous()
        hip()
        ref = eager()
        torch.cuda.synchronize()
        agree = [float((a - b).abs().max() / b.abs().max()) for a, b in
                 ((out['dx'].permute(0, 3, 1, 2), ref[0]), (out['dw'].permute(0, 3, 1, 2), ref[1]), (out['db'], ref[2]))]
        assert max(agree) < 1e-3, (name, agree)            # the two compute the same thing (the tests hold the real bound)
        versions = [('hip', hip), ('torch', eager), ('fwd', fwd)]
        if f16:
            hip3()
            torch.cuda.synchronize()
            agree3 = [float((out3[k_] - out[k_]).abs().max() / out[k_].abs().max()) for k_ in ('dx', 'dw', 'db')]
            assert max(agree3) < 1e-4, (name, agree3)
            versions.append(('f16x3', hip3))
        times = benchlib.alternating(versions, reps, warmup=10)
        med = {k_: benchlib.stats(v)[0] * 1e3 for k_, v in times.items()}
        M, K = B * OH * OW, k * k * cin
        fl = 2.0 * M * cout * K
        print('%-30s %9d %6d %7d | %9.1f %7.1f | %9.1f %7.1f | %9.2f %7.1f'
              % (name, M, cout, K, med['hip'], 2 * fl / med['hip'] / 1e6, med['torch'], 2 * fl / med['torch'] / 1e6,
                 med['hip'] / med['torch'], fl / med['fwd'] / 1e6)
              + (' | %9.1f %7.1f %9.2f' % (med['f16x3'], 2 * fl / med['f16x3'] / 1e6, med['f16x3'] / med['hip']) if f16 else ''), flush=True)
    print('(times are medians of %d runs in us, event-timed one call at a time, launch overhead of the 3 to 6 launches of a call included;'
          ' TF/s = 4 M N K / time for the backward, 2 M N K / time for the forward)' % reps)


def main():
    benchlib.main(__file__, child, out='conv_backward_bench.txt', reps=50, timeout=420,
                  header='# python tools/conv_backward_bench.py --reps %(reps)d --precision %(precision)s   (see the tool for what each column measures)',
                  extra=[('--precision', dict(choices=['f32', 'f16x3'], default='f32'))])


if __name__ == '__main__':
    main()
