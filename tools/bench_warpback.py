#!/usr/bin/env python3
"""The warp-back renderer on the device (mpf_mesh.hip): the time of warpback.warp_back (two renders) at B = 8, 256 x 384, of its parts, and of
the rasteriser's worst case, one face over the whole frame, at the same shape.

    python tools/bench_warpback.py [--rounds 7] [--warmup 2] [--calls 20] [--out profiles/warpback/bench.json]

Device events around `calls` launches in a row, after a warm-up; every figure is the median of the rounds with min and max beside it.  The
scene is a near block on a sloped background at the reference's pose (x = 0.2), so the first render has faces stretched across the block's
edges.  Parts: ops.rgbd_mesh_vertices alone, ops.rasterize_grid alone, and its two halves through the C ABI's `passes` selector on buffers
allocated once: the clear with the z pass (MPF_MESH_PASS_Z), and the resolve pass on the keys that left (MPF_MESH_PASS_RESOLVE); their sum
is the call without its five allocations.  Algorithmic bytes of one render:
the vertex stage reads 16 and writes 32 bytes per pixel; the rasteriser reads 32 bytes per vertex, clears, updates and reads an 8-byte key
per pixel and writes 8 + 4 + 12 + 20 bytes per pixel.  No ROCm baseline exists for pytorch3d's rasteriser: the figures are a record."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpiflow_amd import _lib, ops  # noqa: E402
from mpiflow_amd.warpback import warp_back  # noqa: E402

B, H, W = 8, 256, 384


def scene(b, h, w, seed=1):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    block = (np.abs(x - 0.5) < 0.2) & (np.abs(y - 0.5) < 0.25)
    disp = np.broadcast_to(np.where(block, 0.9, 0.25 + 0.03 * x + 0.02 * y), (b, 1, h, w))
    return np.concatenate([rng.random((b, 3, h, w)), disp], axis=1).astype(np.float32)


def timed(fn, a):
    ms = []
    for r in range(a.warmup + a.rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            ms.append(t0.elapsed_time(t1) / a.calls)
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def raster_halves(verts, attrs, h, w, blur=1e-6):
    """-> (z, resolve): two callables, mpf_rasterize_grid's clear + z pass and its resolve pass, on buffers allocated here"""
    lib = _lib.load()
    B, C, dev = verts.shape[0], attrs.shape[2], verts.device
    pix = torch.empty((B, h, w), dtype=torch.int64, device=dev)
    zbuf = torch.empty((B, h, w), device=dev)
    bary = torch.empty((B, h, w, 3), device=dev)
    out = torch.empty((B, C, h, w), device=dev)
    ws = torch.empty(int(lib.mpf_rasterize_grid_workspace(B, h, w)) // 8, dtype=torch.int64, device=dev)
    keep = (verts, attrs, pix, zbuf, bary, out, ws)

    def call(passes):
        a = _lib.MpfMeshRasterArgs()
        a.verts_ndc, a.attrs, a.pix_to_face, a.zbuf, a.bary, a.out = verts.data_ptr(), attrs.data_ptr(), pix.data_ptr(), zbuf.data_ptr(), bary.data_ptr(), out.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        a.B, a.h, a.w, a.C, a.blur_radius, a.passes = B, h, w, C, blur, passes
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return lambda: (keep, _lib.check(lib.mpf_rasterize_grid(ctypes.byref(a), stream), "mpf_rasterize_grid"))

    z, resolve = call(_lib.MESH_PASS_Z), call(_lib.MESH_PASS_RESOLVE)
    z()
    resolve()
    ref = ops.rasterize_grid(verts, attrs, h, w, blur)
    assert all(torch.equal(x, y) for x, y in zip(ref, (pix, zbuf, bary, out))), "the two halves differ from the whole call"
    return z, resolve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_warpback.py needs a GPU"
    dev = torch.device("cuda:0")
    rgbd = torch.from_numpy(scene(B, H, W)).to(dev)
    image, disp = rgbd[:, :3].contiguous(), rgbd[:, 3:].contiguous()
    cam_int = torch.tensor([[0.58, 0, 0.5], [0, 0.58, 0.5], [0, 0, 1]], device=dev).repeat(B, 1, 1)
    ext = torch.eye(4, device=dev)[:3].repeat(B, 1, 1)
    ext[:, 0, 3] = 0.2
    inv = ext.clone()
    inv[:, 0, 3] = -0.2
    shape = "%dx%dx%d" % (B, H, W)
    px = B * H * W
    out = []

    def put(rec):
        out.append(rec)
        print(json.dumps(rec))

    put(dict(what="warpback.warp_back (two renders)", shape=shape, **timed(lambda: warp_back(image, disp, cam_int, ext, inv), a)))
    put(dict(what="ops.rgbd_mesh_vertices", shape=shape, algorithmic_bytes=48 * px, **timed(lambda: ops.rgbd_mesh_vertices(rgbd, cam_int, ext), a)))
    verts, attrs = ops.rgbd_mesh_vertices(rgbd, cam_int, ext)
    put(dict(what="ops.rasterize_grid (clear, z pass, resolve)", shape=shape, algorithmic_bytes=(32 + 16 + 44) * px,
             **timed(lambda: ops.rasterize_grid(verts, attrs, H, W), a)))
    z, resolve = raster_halves(verts, attrs, H, W)
    put(dict(what="mpf_rasterize_grid, clear + z pass", shape=shape, **timed(z, a)))
    put(dict(what="mpf_rasterize_grid, resolve pass", shape=shape, **timed(resolve, a)))
    one = torch.full((B, H * W, 3), 50.0, device=dev)
    one[..., 2] = 2.0
    q = (H // 2) * W + W // 2
    for i, v in ((q, (9.0, 21.0, 1.0)), (q + W, (9.0, -21.0, 1.5)), (q + W + 1, (-33.0, -21.0, 0.5))):
        one[:, i] = torch.tensor(v, device=dev)
    put(dict(what="ops.rasterize_grid, one face over the whole frame per sample", shape=shape, **timed(lambda: ops.rasterize_grid(one, attrs, H, W), a)))
    z, resolve = raster_halves(one, attrs, H, W)
    put(dict(what="mpf_rasterize_grid, one face over the whole frame: clear + z pass", shape=shape, **timed(z, a)))
    put(dict(what="mpf_rasterize_grid, one face over the whole frame: resolve pass", shape=shape, **timed(resolve, a)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
