"""Per-level A/B of TSPGAN's up-convs in the fp16x2 mode: up-sample + conv against scale + tap conv + fold (ops.upfold3x3), HIP events, 1024 glyphs and one strip (16).
    python tools/upfold_levels.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from marconet_amd import ops, packing as P
dev = "cuda"
def timeit(fn, it=5):
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / it
for n in (1024, 16):
    for (h, cin, c) in ((4, 512, 512), (8, 512, 512), (16, 512, 512), (32, 512, 256)):
        x = P.from_float(torch.randn(1, h, h, cin).expand(n, h, h, cin).contiguous(), P.MX_DTYPE).to(dev)
        w = torch.randn(c, cin, 3, 3, device=dev) * (cin * 9) ** -0.5
        wf, wt = P.pack_conv_weight(w, P.MX_DTYPE), P.pack_tapconv_weight(w, P.MX_DTYPE)
        s = torch.rand(n, cin, device=dev) * 0.5 + 0.5; d = torch.rand(n, c, device=dev) + 0.5; b = torch.randn(c, device=dev) * 0.1; p = torch.rand(n, c, device=dev) * 0.5 + 0.5
        t_up = timeit(lambda: ops.upsample2x(x, scale=s))
        xu = ops.upsample2x(x, scale=s)
        t_cv = timeit(lambda: ops.conv2d(xu, wf, c, 3, 3, (1, 1), (1, 1), out_scale=d, bias=b, act=3, post_scale=p))
        del xu
        t_sc = timeit(lambda: ops.affine_act(x, s))
        xs = ops.affine_act(x, s)
        t_tc = timeit(lambda: ops.conv2d(xs, wt, 9 * c, 1, 1))
        z = ops.conv2d(xs, wt, 9 * c, 1, 1)
        t_fd = timeit(lambda: ops.upfold3x3(z, c, out_scale=d, bias=b, act=3, post_scale=p))
        gb = (z.numel() + n * 4 * h * h * c) * 4 / 1e9
        plan = ops.conv_plan(xs, 9 * c, 1, 1)
        fl = 2.0 * n * h * h * cin * 9 * c
        print("n=%4d %2d->%2d %d->%d: old %.3f ms (ups %.3f + conv %.3f) | new %.3f ms (scale %.3f + tapconv %.3f [plan %d, %.0f TFLOP/s] + fold %.3f [%.2f GB, %.2f TB/s])"
              % (n, h, 2 * h, cin, c, t_up + t_cv, t_up, t_cv, t_sc + t_tc + t_fd, t_sc, t_tc, plan, fl / t_tc / 1e9, t_fd, gb, gb / t_fd), end="", flush=True)
        del z
        # the same with the tap planes in fp32 (conv2d(out_f32=True) + the fold's fp32-plane entry), where the planner accepts it
        from marconet_amd import _lib
        plan32 = ops.conv_plan(xs, 9 * c, 1, 1, algo=_lib.ALGO_FLAG_F32_OUT)
        if plan32 >= 0:
            t_tc32 = timeit(lambda: ops.conv2d(xs, wt, 9 * c, 1, 1, out_f32=True))
            z32 = ops.conv2d(xs, wt, 9 * c, 1, 1, out_f32=True)
            t_fd32 = timeit(lambda: ops.upfold3x3(z32, c, out_scale=d, bias=b, act=3, post_scale=p, out_dtype=P.MX_DTYPE))
            print(" | fp32 planes %.3f ms (tapconv %.3f [plan %d, %.0f TFLOP/s] + fold %.3f [%.2f TB/s])"
                  % (t_sc + t_tc32 + t_fd32, t_tc32, plan32, fl / t_tc32 / 1e9, t_fd32, gb / t_fd32), flush=True)
            del z32
        else:
            print(" | fp32 planes: refused (%d)" % plan32, flush=True)
        del xs, x
