#!/usr/bin/env python
"""Wall time of Model.report(with_greedy=True) at config 2 (B = 32, k = 10 + 5 held-out demos, 8x8x16 frames, T = 20,
L = 50) with the Karel program metrics on the host (D2P_HOST_PROGRAM_METRICS=1) and on the device (=0), and the
d2p_karel_exec launch alone (events).

The teacher-forced logits are replaced by a mix of ground truth, mutated programs and token soup so that rows of every
kind are executed: ground truth, one action swapped for another, token soup (an untrained model's predictions are nearly all syntax errors, which the metrics skip).  Prints one
JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demo2program_amd import build, kernels as K  # noqa: E402


def mixed_logits(batch, rng):
    gt, gl = batch['program_tokens'], batch['program_len'].reshape(-1).astype(np.int64)
    B, L = gt.shape
    tok = gt.copy()
    for i in range(B):
        acts = np.flatnonzero((gt[i, :gl[i]] >= 4) & (gt[i, :gl[i]] <= 8))     # move ... putMarker
        if i % 4 in (1, 2) and acts.size:
            j = acts[rng.randint(acts.size)]              # another action: still a program, executed on every demo
            tok[i, j] = 4 + (gt[i, j] - 4 + rng.randint(1, 5)) % 5
        elif i % 4 == 3:
            tok[i] = rng.randint(0, 50, L)
    onehot = np.zeros((L, B, 50), np.float32)
    onehot[np.arange(L)[:, None], np.arange(B)[None, :], tok.T] = 10.0
    return torch.from_numpy(onehot).cuda()


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    build.build_library()
    from demo2program_amd.config import make_config
    from demo2program_amd.karel_env.generator import sample_batch
    from demo2program_amd.models import program_metrics as PM
    from demo2program_amd.models.model_full import Model
    cfg = make_config('karel', batch_size=32, k=10, test_k=5)
    m = Model(cfg, is_train=False)
    rng = np.random.RandomState(0)
    res = {'host_s': [], 'device_s': [], 'kernel_us': []}
    for i in range(args.batches):
        batch = sample_batch(cfg, seed=100 + i)
        batch['s_h'] = batch['s_h'].astype(np.uint8)
        m.forward(m.get_feed_dict(batch, is_training=False))
        m._ctx['dp']['logits'].copy_(mixed_logits(batch, rng))
        for mode, key in (('1', 'host_s'), ('0', 'device_s')):
            os.environ['D2P_HOST_PROGRAM_METRICS'] = mode
            m.report(with_greedy=True)                              # warm-up
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.report(with_greedy=True)
                ts.append(time.perf_counter() - t0)
            res[key].append(float(np.median(ts)))
        # the launch alone: one program set on both demo sets, as Model.report issues it
        B, k, T = cfg.batch_size, cfg.k, cfg.max_demo_len
        st = Model.sequence_stats(m.pred_program.cpu().numpy(), batch['program'],
                                  batch['program_len'].reshape(-1), batch['program_len'].reshape(-1))
        L = st['pred_tokens'].shape[1]
        tok = torch.from_numpy(st['pred_tokens'].astype(np.int32)).cuda()
        plen = torch.from_numpy(batch['program_len'].reshape(-1).astype(np.int32)).cuda()
        same = torch.from_numpy(st['is_same_seq'].astype(np.int32)).cuda()
        demos = m._feed['s_h'].view(B, k, T, cfg.h, cfg.w, -1)
        dlen = m._feed['demo_len'].view(B, k)
        tdem = torch.from_numpy(batch['test_s_h'].astype(np.uint8)).cuda()
        tlen = torch.from_numpy(batch['test_demo_len'].astype(np.int32)).cuda()
        ws = torch.empty(max(K.call.d2p_karel_exec_ws_bytes(B, L, cfg.h, cfg.w, 16), 4) // 4, dtype=torch.int32,
                         device='cuda')
        outs = [torch.empty(n, dtype=torch.int32, device='cuda') for n in (B, B * 15, B * 15, B * 2)]
        s = torch.cuda.current_stream().cuda_stream

        def launch():
            K.call.d2p_karel_exec(B, L, tok.data_ptr(), L, plen.data_ptr(), same.data_ptr(), cfg.h, cfg.w, 16, 6,
                                  k, T, demos.data_ptr(), demos.shape[5], dlen.data_ptr(),
                                  5, T, tdem.data_ptr(), 16, tlen.data_ptr(),
                                  *[o.data_ptr() for o in outs], None, None, None, 0, ws.data_ptr(), ws.numel() * 4, s)
        launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20
        e0.record()
        for _ in range(n):
            launch()
        e1.record()
        torch.cuda.synchronize()
        res['kernel_us'].append(e0.elapsed_time(e1) * 1e3 / n)
        dev = PM.karel_device_metrics(st['pred_tokens'], batch['program_len'].reshape(-1), st['is_same_seq'],
                                      demos, dlen, tdem, tlen, make_error=False)
        res.setdefault('rows_run', []).append(int((dev['exec_len'] > 0).any(axis=1).sum()))
    out = {'report_with_greedy_host_s': float(np.median(res['host_s'])),
           'report_with_greedy_device_s': float(np.median(res['device_s'])),
           'karel_exec_launch_us': float(np.median(res['kernel_us'])),
           'per_batch': res}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
