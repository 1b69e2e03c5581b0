#!/usr/bin/env python3
"""Time one GradAccumulator.add over the full model's tensor list (ConvNeXt-Base configuration, seeded gradients of the parameters'
shapes; no forward is run) on the device, next to torch._foreach_add_ + torch.nn.utils.clip_grad_norm_ over the same tensors.

    python scripts/grad_accum_time.py [--repeats 40] [--calls 5] [--warmup 6] [--out FILE]

Three figures, each the median over `--repeats` windows of `--calls` calls between two device events, after `--warmup` calls:
  * add(grads, scale, clip_norm) without a group in the steady state of a window (a = a + scale * g, norm, a *= coef): 3 launches;
  * the two-phase form of a group of two ranks with the collective itself left out (stage = scale / 2 * g; a = a + stage, norm,
    a *= coef): 5 launches -- what a rank spends around the all_reduce, not the all_reduce;
  * the baseline: torch._foreach_add_(acc, grads, alpha=scale) and torch.nn.utils.clip_grad_norm_ over separate tensors.
Bytes per call are what the algorithm needs: a read and written and g read by the accumulation, a read and written by the scaling
(5 x 4 bytes per element); the two-phase form also writes and reads stage (7 x 4).  The bandwidth figure is bytes over the call time,
host table build included -- a whole-call rate, not a kernel's share of peak.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HBM_ACHIEVABLE = 6.29e12     # bytes / s: a float4 copy on an MI355X (79 % of the 8 TB/s of the data sheet)


def windows(fn, repeats, calls):
    """-> the time of one call in seconds per window, from device events around `calls` calls."""
    import torch
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 20:
        raise SystemExit("at least 20 timed repeats")
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    import torch

    from givepose_amd import GradAccumulator, Ranger, _lib
    from optim_step_time import setup
    if not torch.cuda.is_available():
        raise SystemExit("grad_accum_time.py needs the GPU: a time from anywhere else says nothing")
    net, grads = setup()
    opt = Ranger(net)
    idx = sorted({opt._index[n] for n in grads})
    n_elem = sum(opt.params[i].numel() for i in idx)
    scale, clip = 0.5, 5.0
    say(f"device: {torch.cuda.get_device_name(0)}; {len(idx)} tensors with a gradient of {len(opt.params)}, {n_elem / 1e6:.1f} M elements; "
        f"median of {args.repeats} windows of {args.calls} calls after {args.warmup} warm-up calls")

    def report(what, times, nbytes, launches):
        t = statistics.median(times)
        say(f"{what}: {t * 1e3:.3f} ms per call (min {min(times) * 1e3:.3f}, max {max(times) * 1e3:.3f}), {launches} launches")
        say(f"    {nbytes / 1e9:.2f} GB per call needed -> {nbytes / t / 1e12:.2f} TB/s, {nbytes / t / HBM_ACHIEVABLE:.2f} of the "
            f"{HBM_ACHIEVABLE / 1e12:.2f} TB/s a float4 copy achieves on this device")
        return t

    acc = GradAccumulator(opt)
    one = lambda: acc.add(grads, scale=scale, clip_norm=clip)
    for _ in range(args.warmup):
        one()
    t_one = report("add with clip, no group (gpc_grad_accumulate, host table build included)", windows(one, args.repeats, args.calls),
                   n_elem * 4 * 5, _lib.GPC_ACCUM_LAUNCHES)

    class NoCollective(GradAccumulator):          # the two phases of a group of two ranks around an all_reduce that is not issued
        def _world(self, group):
            return 2

        def _all_reduce(self, group):
            pass
    two = NoCollective(opt)
    both = lambda: two.add(grads, scale=scale, clip_norm=clip, group="left out")
    for _ in range(args.warmup):
        both()
    report("two-phase add with clip, collective left out", windows(both, args.repeats, args.calls), n_elem * 4 * 7, 2 * _lib.GPC_ACCUM_LAUNCHES - 1)

    # the baseline: PyTorch's own multi-tensor ops over the same tensors as separate allocations
    params = [torch.nn.Parameter(torch.empty_like(opt.params[i]), requires_grad=False) for i in idx]
    for p in params:
        p.grad = torch.zeros_like(p)
    accs, gs = [p.grad for p in params], [grads[opt.param_names[i]] for i in idx]

    def base():
        torch._foreach_add_(accs, gs, alpha=scale)
        torch.nn.utils.clip_grad_norm_(params, clip)
    for _ in range(args.warmup):
        base()
    t_base = report("torch._foreach_add_ + torch.nn.utils.clip_grad_norm_, same tensors", windows(base, args.repeats, args.calls), n_elem * 4 * 5, "PyTorch's")
    say(f"baseline / add without a group: {t_base / t_one:.2f}")


if __name__ == "__main__":
    main()
