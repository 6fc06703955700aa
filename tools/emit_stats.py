#!/usr/bin/env python
"""What phase D of the default backward sends to its LDS accumulator, per wave and chunk, on the bench scenes -- and what the
measured cost of an LDS float add (tools/calib/lds_atomic_calib.hip -> profiles/lds_atomic_calibration.jsonl) makes of it.

    python tools/emit_stats.py [--config cfg2 cfg4] [--max-tiles 1500] [--calibration profiles/lds_atomic_calibration.jsonl]

Runs the forward of each configuration, reads the tile lists, n_contrib and the blend masks it left (the masks straight out of
the binning scratch: they sit in front of hit_base and hit_valid at the end of its fixed part, dm2_state.h BinningState::carve;
checked against hit_valid itself and against the forward's count of blended pairs),
and replays on the host the backward's chunk cut (dm2_backward_fast.hip: walk from the tile's deepest live entry, <= 30
candidates, the leading ones whose pairs fit 256 lanes) and its pair-lane map (face-major: a face is a run of lanes).  Per
wave-chunk: the emit lanes with one emit per (face, 16-lane row) and with one per (face, wave), and how many lanes of one add
instruction share their address (a face that emits from k rows).  Pairs behind a pixel's last contributor count as active here.

The calibration prices an add instruction by its active lanes (cycles = c0 + lanes x per-lane cost, the per-lane cost a little
higher where lanes share an address); predicted LDS-array cycles per wave-chunk of the 29 adds:
  today     one emit per (face, row)
  (a)       one emit per (face, wave)
  (b)       staged: the emit lanes store 29 values + a row index with 8 ds_write_b128, dense lanes (emit, component) read them
            back (ds_read_b32) and add; same-face emits summed first, so its add lanes are (a)'s -- packed into fewer instructions
  (a)+(b)   both
  (a)+stores  one emit per (face, wave); a face with lanes in one wave only has ONE emit in the block and stores (ds_write_b32,
            priced per instruction), a face that crosses into a neighbouring wave adds"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAND, LANES, ADDS = 30, 256, 29


def align(n, a=256):
    return (n + a - 1) // a * a


def forward_state(cfg, dev):
    import bench
    from dmesh2_renderer_amd import _C
    from dmesh2_renderer_amd.sharding import BandShardedOp
    args, _, _, _ = bench.build_inputs(cfg, dev, 0, 1)
    op = BandShardedOp(args, 1, 0)
    op.forward()
    out = op.fwd
    torch.cuda.synchronize()
    assert _C.last_forward_mode() == _C.FWD_POOL
    R, bin_buf, img_buf = out[0], out[8], out[9]
    B, H, W = out[2].shape
    N, Tn = B * H * W, _C._tiles(B, W, H)
    ranges = _C.debug_fetch(0, N, Tn, R, img_buf, torch.int32, Tn * 2).cpu().numpy().view(np.uint32).reshape(Tn, 2).astype(np.int64)
    nc = _C.debug_fetch(4, N, Tn, R, img_buf, torch.int32, N).cpu().numpy().view(np.uint32).reshape(B, H, W)
    fixed = _C.load_library().dm2_scratch_bytes(_C.SCRATCH_BINNING, R, Tn)
    off_valid = fixed - 256 - 32
    off_base = off_valid - align(4 * R)
    off_masks = off_base - align(32 * R)
    assert off_valid % 256 == 0 and off_masks >= 0
    hv = _C.debug_fetch(9, N, Tn, R, bin_buf, torch.int32, 4).cpu().numpy()
    assert np.array_equal(bin_buf[off_valid:off_valid + 16].cpu().numpy().view(np.int32), hv), "the scratch layout has changed"
    masks = bin_buf[off_masks:off_masks + 32 * R].cpu().numpy().view(np.uint64).reshape(R, 4)
    # (no debug_fetch item returns the masks; two checks keep a changed layout from going unnoticed: hit_valid read both ways
    # above, and every mask bit is a blended pair with a pool slot -- their number is the forward's own count, hit_valid[1])
    gx, gy = (W + 15) // 16, (H + 15) // 16
    pad = np.zeros((B, gy * 16, gx * 16), np.uint32)
    pad[:, :H, :W] = nc
    max_lc = pad.reshape(B, gy, 16, gx, 16).max(axis=(2, 4)).reshape(Tn)
    return ranges, max_lc, masks


def popcount64(x):
    x = x.astype(np.uint64)
    out = np.zeros(x.shape, np.int64)
    for s in range(0, 64, 8):
        out += np.unpackbits(((x >> np.uint64(s)) & np.uint64(0xFF)).astype(np.uint8)[..., None], axis=-1).sum(-1).astype(np.int64)
    return out


def replay(ranges, max_lc, masks, max_tiles, seed=0):
    """-> per busy wave-chunk: emit lanes today (per row), with (a) (per wave), those of (a) whose face has lanes in another wave
    too (they add, the others store); multiplicity histogram, chunk count."""
    tiles = np.flatnonzero((ranges[:, 1] > ranges[:, 0]) & (max_lc > 0))
    if max_tiles and len(tiles) > max_tiles:
        tiles = np.sort(np.random.RandomState(seed).choice(tiles, max_tiles, replace=False))
    lanes_row, lanes_wave, lanes_cross, mult, chunks, idle = [], [], [], np.zeros(5, np.int64), 0, 0
    w4 = np.arange(4)
    for t in tiles:
        r0, r1 = ranges[t]
        total = int(min(max_lc[t], r1 - r0))
        cnt = popcount64(masks[r0:r0 + total][::-1]).sum(axis=1)                  # pairs per entry, walk order
        base = 0
        while base < total:
            c = cnt[base:base + CAND]
            cum = np.cumsum(c)
            n = max(1, int((cum <= LANES).sum()))
            c, end = c[:n], np.minimum(cum[:n], LANES)                             # (a lone face over 256 cannot be: <= 256 pixels)
            start = end - c
            live = c > 0
            first_row, last_row = start[live] // 16, (end[live] - 1) // 16
            # rows of thread wave w that face j has lanes in
            k = np.clip(np.minimum(last_row[:, None], 4 * w4 + 3) - np.maximum(first_row[:, None], 4 * w4) + 1, 0, 4)
            busy = k.sum(axis=0) > 0
            lanes_row += k.sum(axis=0)[busy].tolist()
            lanes_wave += (k > 0).sum(axis=0)[busy].tolist()
            lanes_cross += ((k > 0) & ((k > 0).sum(axis=1) > 1)[:, None]).sum(axis=0)[busy].tolist()   # faces with lanes in another wave too
            mult += np.bincount(k[k > 0], minlength=5)[:5]
            idle += int((~busy).sum())
            chunks += 1
            base += n
    return np.array(lanes_row), np.array(lanes_wave), np.array(lanes_cross), mult, chunks, idle, len(tiles)


def calibration(path):
    """-> c0, per-lane cost at 1, 2, 4 lanes per address, ds_write_b128, ds_read_b32 (LDS cycles per wave-instruction, from the
    wall clock at 16 waves per CU)"""
    rows = [json.loads(l) for l in open(path) if '"kind"' in l]
    at = lambda kind, n, m=1, banks="distinct": next(r["lds_cycles_per_instr_wall"] for r in rows if r["kind"] == kind and r["waves_per_cu"] == 16
                                                     and r["active_lanes"] == n and r["lanes_per_address"] == m and r["banks"] == banks)
    per1 = (at("ds_add_f32", 64) - at("ds_add_f32", 1)) / 63.0
    c0 = at("ds_add_f32", 1) - per1
    per = {1: per1, 2: (at("ds_add_f32", 64, 2) - c0) / 64.0, 4: (at("ds_add_f32", 64, 4) - c0) / 64.0}
    per[3] = 0.5 * (per[2] + per[4])
    return c0, per, at("ds_write_b128", 10), at("ds_read_b32", 64), at("ds_add_f32", 10, 1, "one") / at("ds_add_f32", 10), at("ds_write_b32", 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["cfg2", "cfg4"])
    ap.add_argument("--max-tiles", type=int, default=1500)
    ap.add_argument("--calibration", default=os.path.join(ROOT, "profiles", "lds_atomic_calibration.jsonl"))
    opt = ap.parse_args()
    c0, per, wr128, rd32, one_bank, wr32 = calibration(opt.calibration)
    print(json.dumps(dict(calibration=dict(add_c0=round(c0, 2), add_per_lane={k: round(v, 2) for k, v in per.items()},
                                           ds_write_b128=wr128, ds_write_b32=wr32, ds_read_b32=rd32, one_bank_over_distinct=round(one_bank, 3)))))
    dev = torch.device("cuda", 0)
    for cfg in opt.config:
        lr, lw, lx, mult, chunks, idle, ntiles = replay(*forward_state(cfg, dev), opt.max_tiles)
        n = len(lr)
        shared = mult[2] * 2 + mult[3] * 3 + mult[4] * 4
        # today: per instruction c0 + every emit lane at the cost of its address' multiplicity
        today = ADDS * (c0 * n + sum(mult[k] * k * per[k] for k in (1, 2, 3, 4))) / n
        a = ADDS * (c0 + per[1] * lw.mean())
        # (a) + stores: 29 ds_write_b32 where a face of the wave owns its row, 29 adds of the crossing faces' lanes where there are any
        own = ADDS * (wr32 * (lw > lx) + (c0 + per[1] * lx) * (lx > 0)).mean()
        dense = lambda e: (c0 * np.ceil(ADDS * e / 64.0) + per[1] * ADDS * e + 8 * wr128 + rd32 * 2 * np.ceil(32 * e / 64.0)).mean()
        print(json.dumps(dict(
            config=cfg, tiles=ntiles, chunks=chunks, busy_wave_chunks=n, idle_wave_chunks=idle,
            emit_lanes_per_face_row=round(float(lr.mean()), 2), emit_lanes_per_face_wave=round(float(lw.mean()), 2),
            emit_lanes_ratio=round(float(lw.sum() / lr.sum()), 3), emit_lanes_that_must_add=round(float(lx.mean()), 2),
            share_of_row_emit_lanes_sharing_an_address=round(float(shared / lr.sum()), 3),
            faces_by_rows_emitted_from={k: int(mult[k]) for k in (1, 2, 3, 4)},
            predicted_lds_cycles_per_wave_chunk=dict(today=round(float(today)), a=round(float(a)), b=round(float(dense(lw))),
                                                     a_and_b=round(float(dense(lw))), a_and_stores=round(float(own))))))


if __name__ == "__main__":
    main()
