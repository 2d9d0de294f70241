"""The f16x3 training forward (one srcnn_conv2d_forward_f16x3 call) against the exact-fp32 engine's forward of the same layer.

    python tools/conv_forward_f16x3_bench.py [--out profiles/conv_forward_f16x3_bench.txt] [--reps 50]

Shapes: tools/conv_backward_bench.py's layer list (the trainable trunk and head at B = 1, one 600 x 1987 image).
  * fp32  : srcnn_conv2d, precision 0, heuristic plan, bias + ReLU -- what forward_train runs by default;
  * f16x3 : srcnn_conv2d_forward_f16x3 on the same tensors, everything the call issues: the clear of the scale words, the max|w|
            and max|x| passes, the weight split and the implicit GEMM (weights change every step, so all of it is per call).
The two ALTERNATE inside every round of one process; whole calls are timed between device events; medians of --reps after 10
untimed rounds.  FLOPs: 2 M N K.  Runner and timer: tools/benchlib.py."""
import benchlib
from conv_backward_bench import LAYERS


def child(reps):
    import torch
    from stereo_rcnn_amd import engine
    dev = benchlib.device()
    print('%-30s %9s %6s %7s | %9s %7s | %9s %7s | %10s' % ('layer', 'M', 'N', 'K', 'fp32 us', 'TF/s', 'f16x3 us', 'TF/s', 'f16x3/fp32'))
    for name, B, H, W, cin, cout, k, s, p in LAYERS:
        gen = torch.Generator().manual_seed(1)
        OH, OW = engine.conv_out_hw(H, W, k, k, s, p)
        x = torch.randn(B, H, W, cin, generator=gen).to(dev)
        w = (torch.randn(cout, k, k, cin, generator=gen) / float(k * k * cin) ** 0.5).to(dev)
        cw = engine.ConvW(w, torch.randn(cout, generator=gen).to(dev), k, k, s, p, True)
        y32, y16 = torch.empty(B, OH, OW, cout, device=dev), torch.empty(B, OH, OW, cout, device=dev)

        def fp32():
            engine.conv2d(cw, x, B, H, W, y32, OH, OW, precision='f32', plan=(0, 0, 0, 0, 0))

        def f16x3():
            engine.conv2d_train_f16x3(cw, x, B, H, W, y16, OH, OW)

        fp32(), f16x3()
        torch.cuda.synchronize()
        agree = float((y16 - y32).abs().max() / y32.abs().max())
        assert agree < 1e-4, (name, agree)            # the two compute the same thing (the tests hold the real bound)
        times = benchlib.alternating([('fp32', fp32), ('f16x3', f16x3)], reps, warmup=10)
        med = {k_: benchlib.stats(v)[0] * 1e3 for k_, v in times.items()}
        M, K = B * OH * OW, k * k * cin
        fl = 2.0 * M * cout * K
        print('%-30s %9d %6d %7d | %9.1f %7.1f | %9.1f %7.1f | %10.2f'
              % (name, M, cout, K, med['fp32'], fl / med['fp32'] / 1e6, med['f16x3'], fl / med['f16x3'] / 1e6, med['f16x3'] / med['fp32']),
              flush=True)
    print('(times are medians of %d runs in us, event-timed one call at a time, launch overhead of the 5 launches of an f16x3 call included;'
          ' TF/s = 2 M N K / time)' % reps)


def main():
    benchlib.main(__file__, child, out='conv_forward_f16x3_bench.txt', reps=50, timeout=420,
                  header='# python tools/conv_forward_f16x3_bench.py --reps %(reps)d   (see the tool for what each column measures)')


if __name__ == '__main__':
    main()
