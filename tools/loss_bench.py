#!/usr/bin/env python
"""Times fpd_loss_ohkm (csrc/loss_ohkm.hip, two launches) against fpd_loss (csrc/loss_adam.hip, one launch) at one shape, on the
same buffers, in alternating batches of back-to-back calls between two device events (so both see the same machine state).

    python tools/loss_bench.py [--batch 32 --joints 16 --size 64 --stacks 4 --dtype bf16 --topk 8 --rounds 7 --calls 200] [--out FILE]

Prints one line per round and a summary: median us per call of either, their ratio, and the budget the new path was given
(twice the fpd_loss time: it reads the maps twice; plus one launch gap, reported separately as the time of an empty-handed
second launch is not measured here).

    python tools/loss_bench.py --kl 1.0 [--step] [...]

times fpd_loss_kl (csrc/loss_kl.hip, two launches; pose term MSE, distillation term KL at that temperature) instead, by the same
protocol, and reports the launch gap as the difference of the two entry points on an 8x8 map of one image, where neither has
work to speak of.  --step adds the whole train step of the benchmark pair (hourglass 128 x 4 student, 256 x 8 teacher, 256x256
images): FusedFPDStep(kl=(None, T)) against the default step, each sample in a process of its own, the two kinds alternating.

    python tools/loss_bench.py --digest [--kl T] [...]

times nothing: one call each of fpd_loss, fpd_loss_ohkm, fpd_loss_kl (None, T) and fpd_loss_kl (T, T) on the same seeded inputs,
and one line per call with the SHA-256 of everything it wrote.  Two builds of the library (FPD_AMD_LIB) print the same lines
or do not compute the same bytes."""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fpd_amd import runtime as R  # noqa: E402


def launch_gap(kk, dt, tdt, dev, timed, a):
    """fpd_loss (one launch) against fpd_loss_kl (two) on one 8x8 map: the difference is one launch gap"""
    lib, st = R.lib(), R.current_stream()
    J = kk.base.J
    o, d, t = (torch.zeros(1, 8, 8, J, dtype=tdt, device=dev) for _ in range(3))
    tg, w = torch.zeros(1, J, 8, 8, device=dev), torch.ones(1, J, device=dev)
    losses = torch.zeros(2, dtype=torch.float64, device=dev)
    scratch = torch.empty(1 << 12, dtype=torch.float64, device=dev)
    s = R.LossKlT()
    b = s.base
    b.B, b.J, b.H, b.W, b.S, b.dtype, b.target_nchw, b.alpha, b.grad_scale = 1, J, 8, 8, 1, dt, 1, 0.5, 1.0
    b.out[0], b.dout[0] = o.data_ptr(), d.data_ptr()
    b.teacher, b.target, b.weight, b.losses = t.data_ptr(), tg.data_ptr(), w.data_ptr(), losses.data_ptr()
    s.kl_pose, s.kl_kd, s.temp_pose, s.temp_kd = 0, 1, 1.0, a.kl
    s.scratch, s.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
    one = lambda: R.check(lib.fpd_loss(s.base, st), 'fpd_loss')
    two = lambda: R.check(lib.fpd_loss_kl(s, st), 'fpd_loss_kl')
    timed(one, 20), timed(two, 20)
    u1, u2 = [], []
    for _ in range(a.rounds):
        u1.append(timed(one, a.calls)), u2.append(timed(two, a.calls))
    m1, m2 = statistics.median(u1), statistics.median(u2)
    return ['launch gap: one 8x8 map  fpd_loss %.2f us (1 launch)  fpd_loss_kl %.2f us (2 launches)  difference %.2f us' % (m1, m2, m2 - m1)]


def kl_args(base, kl_pose, temp, dev):
    """fpd_loss_kl_t over the maps of `base`: distillation term KL at `temp`, pose term too if kl_pose; and its scratch (keep it alive)"""
    kk = R.LossKlT()
    C.memmove(C.byref(kk.base), C.byref(base), C.sizeof(R.LossT))
    kk.kl_pose, kk.kl_kd, kk.temp_pose, kk.temp_kd = int(kl_pose), 1, temp if kl_pose else 1.0, temp
    nbytes = R.lib().fpd_loss_kl_scratch_bytes(kk.base)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    kk.scratch, kk.scratch_bytes = scratch.data_ptr(), nbytes
    return kk, scratch


def digest(a, k, losses, douts, masks, dev):
    """--digest: what every entry point writes on the seeded inputs, as SHA-256 (default temperature 2)"""
    lib, st, T = R.lib(), R.current_stream(), a.kl or 2.0
    sha = lambda t: hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
    (k1, s1), (k2, s2) = kl_args(k.base, False, T, dev), kl_args(k.base, True, T, dev)
    for name, fn, arg in (('fpd_loss', lib.fpd_loss, k.base), ('fpd_loss_ohkm topk=%d' % a.topk, lib.fpd_loss_ohkm, k),
                          ('fpd_loss_kl (None, %g)' % T, lib.fpd_loss_kl, k1), ('fpd_loss_kl (%g, %g)' % (T, T), lib.fpd_loss_kl, k2)):
        for t in [losses, masks] + douts:
            t.zero_()
        R.check(fn(arg, st), name)
        torch.cuda.synchronize()
        print('%-24s losses %s  dout %s%s' % (name, sha(losses), ' '.join(sha(d) for d in douts),
                                             '  masks ' + sha(masks) if fn is lib.fpd_loss_ohkm else ''))


def step_child(a, dev):
    """One train step of the benchmark pair, alone in this process: prints `STEP_MS <ms per step> ...` for a.step_rounds samples"""
    from fpd_amd import executor as E, synth
    from fpd_amd.lib.models import hourglass

    class AD(dict):
        __getattr__ = dict.__getitem__
    cfg = lambda f, s: AD(MODEL=AD(NUM_JOINTS=16, DTYPE=a.dtype, EXTRA=AD(NUM_FEATURES=f, NUM_STACKS=s, NUM_BLOCKS=1)))
    B, J, H, W = a.batch, 16, 256, 256
    torch.manual_seed(1)
    student = hourglass.get_pose_net(cfg(128, 4), is_train=True).to(dev)
    torch.manual_seed(2)
    teacher = hourglass.get_pose_net(cfg(256, 8), is_train=False).to(dev)
    x, tg, tw = synth.make_batch(1000, B, J, (W, H), (W // 4, H // 4))
    cal = E.GraphInstance(teacher.device_state(), teacher.cfg_hg, B, H, W, train=True).finalize()
    cal.image().copy_(x)
    cal.run('prep'); cal.run('fwd')
    cal.calibrate_running_stats()
    del cal
    torch.cuda.empty_cache()
    st = E.FusedFPDStep(student.device_state(), student.cfg_hg, teacher.device_state(), teacher.cfg_hg, B, H, W,
                        alpha=0.5, lr=2.5e-4, kl=(None, a.kl) if a.step_child == 'kl' else None)
    st.set_batch(x, tg, tw)
    st.run_pipelined(5)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.step_rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st.run_pipelined(a.step_steps)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.step_steps)
    print('STEP_MS %s launches %d pose %.6g kd %.6g' % (' '.join('%.4f' % v for v in ms), st.launches_per_step()['total'], *st.losses()[:2]))


def step_times(a):
    """The benchmark pair's train step with the default loss and with kl=(None, T).  Several steps built in ONE process are not
    comparable (the later ones run up to 50 % slower whatever their loss: measured, an A/A of two default steps shows it), so
    every sample is a fresh child process that builds one step, and the two kinds alternate."""
    import subprocess
    lines = ['# train step of the benchmark pair, B=%d %s: ms per step, %d pipelined steps per sample, %d samples per process, '
             'processes alternating' % (a.batch, a.dtype, a.step_steps, a.step_rounds)]
    ms, tail = {'default': [], 'kl': []}, {}
    for r in range(a.step_procs):
        for kind in ('default', 'kl'):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--kl', str(a.kl), '--step-child', kind, '--batch', str(a.batch),
                                  '--dtype', a.dtype, '--step-rounds', str(a.step_rounds), '--step-steps', str(a.step_steps)],
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit('step child %s failed:\n%s' % (kind, out.stderr[-2000:]))
            f = [l for l in out.stdout.splitlines() if l.startswith('STEP_MS')][0].split()
            n = f.index('launches')
            ms[kind] += [float(v) for v in f[1:n]]
            tail[kind] = ' '.join(f[n:])
            lines.append('process %d  %-7s %s' % (r, kind, ' '.join(f[1:n])))
    m0, m1 = statistics.median(ms['default']), statistics.median(ms['kl'])
    lines.append('median  default %.3f ms (min %.3f max %.3f)  kl=(None, %g) %.3f ms (min %.3f max %.3f)  difference %+.1f us'
                 % (m0, min(ms['default']), max(ms['default']), a.kl, m1, min(ms['kl']), max(ms['kl']), (m1 - m0) * 1e3))
    lines.append('default: %s;  kl: %s' % (tail['default'], tail['kl']))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--joints', type=int, default=16)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--stacks', type=int, default=4)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--topk', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--kl', type=float, default=None, metavar='T', help='time fpd_loss_kl (kd term KL at temperature T) instead of fpd_loss_ohkm')
    ap.add_argument('--step', action='store_true', help='with --kl: also time the whole train step of the benchmark pair with and without the KL term')
    ap.add_argument('--step-rounds', type=int, default=3)
    ap.add_argument('--step-procs', type=int, default=3, help='processes per kind of step')
    ap.add_argument('--step-child', default='', choices=['', 'default', 'kl'], help=argparse.SUPPRESS)
    ap.add_argument('--step-steps', type=int, default=20)
    ap.add_argument('--digest', action='store_true', help='no timing: one call of every entry point and the SHA-256 of what it wrote')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'loss_bench needs the GPU'
    dev = torch.device('cuda:0')
    if a.step_child:
        return step_child(a, dev)
    B, J, H, S = a.batch, a.joints, a.size, a.stacks
    dt, tdt = (R.BF16, torch.bfloat16) if a.dtype == 'bf16' else (R.F32, torch.float32)
    gen = torch.Generator().manual_seed(0)
    outs = [torch.randn(B, H, H, J, generator=gen).to(tdt).to(dev) for _ in range(S)]
    douts = [torch.empty_like(o) for o in outs]
    teacher = torch.randn(B, H, H, J, generator=gen).to(tdt).to(dev)
    target = torch.rand(B, J, H, H, generator=gen).to(dev)
    weight = torch.rand(B, J, generator=gen).to(dev)
    losses = torch.zeros(2, dtype=torch.float64, device=dev)
    k = R.LossOhkmT()
    for s in (k.base, ):
        s.B, s.J, s.H, s.W, s.S, s.dtype, s.target_nchw, s.alpha, s.grad_scale = B, J, H, H, S, dt, 1, 0.5, 1.0
        for i in range(S):
            s.out[i], s.dout[i] = outs[i].data_ptr(), douts[i].data_ptr()
        s.teacher, s.target, s.weight, s.losses = teacher.data_ptr(), target.data_ptr(), weight.data_ptr(), losses.data_ptr()
    k.topk_pose = k.topk_kd = a.topk
    nbytes = R.lib().fpd_loss_ohkm_scratch_bytes(k.base)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    masks = torch.zeros(S * 2 * B, dtype=torch.int32, device=dev)
    k.scratch, k.scratch_bytes, k.masks = scratch.data_ptr(), nbytes, masks.data_ptr()
    if a.digest:
        return digest(a, k, losses, douts, masks, dev)
    lib, st = R.lib(), R.current_stream()
    new = 'fpd_loss_ohkm' if a.kl is None else 'fpd_loss_kl'
    calls = {'fpd_loss': lambda: R.check(lib.fpd_loss(k.base, st), 'fpd_loss'),
             'fpd_loss_ohkm': lambda: R.check(lib.fpd_loss_ohkm(k, st), 'fpd_loss_ohkm')}
    if a.kl is not None:
        kk, kscratch = kl_args(k.base, False, a.kl, dev)
        del calls['fpd_loss_ohkm']
        calls['fpd_loss_kl'] = lambda: R.check(lib.fpd_loss_kl(kk, st), 'fpd_loss_kl')

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for fn in calls.values():                   # warm-up: code objects loaded, caches in their steady state
        timed(fn, 20)
    lines = ['# loss_bench B=%d J=%d %dx%d S=%d %s %s: us per call, %d back-to-back calls per sample, alternating'
             % (B, J, H, H, S, a.dtype, 'topk=%d' % a.topk if a.kl is None else 'kl T=%g (pose MSE, kd KL)' % a.kl, a.calls)]
    us = {n: [] for n in calls}
    for r in range(a.rounds):
        for n, fn in calls.items():
            us[n].append(timed(fn, a.calls))
        lines.append('round %d  fpd_loss %.2f us  %s %.2f us' % (r, us['fpd_loss'][-1], new, us[new][-1]))
    m0, m1 = statistics.median(us['fpd_loss']), statistics.median(us[new])
    traffic = (S + 1) * B * H * H * J * (2 if a.dtype == 'bf16' else 4) + B * J * H * H * 4
    lines.append('median  fpd_loss %.2f us (min %.2f max %.2f)  %s %.2f us (min %.2f max %.2f)  ratio %.2f  budget 2 x fpd_loss = %.2f us (+ one launch gap)'
                 % (m0, min(us['fpd_loss']), max(us['fpd_loss']), new, m1, min(us[new]), max(us[new]), m1 / m0, 2 * m0))
    lines.append('bytes read per pass over the maps %.1f MB, gradients written %.1f MB; library %s'
                 % (traffic / 1e6, S * B * H * H * J * (2 if a.dtype == 'bf16' else 4) / 1e6, R.lib_sha16()))
    if a.kl is not None:
        lines += launch_gap(kk, dt, tdt, dev, timed, a)
        if a.step:
            lines += step_times(a)
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
