#!/usr/bin/env python3
"""Timing of the mesh front end (gldm_mesh_sample_surface in csrc/mesh_sample.hip, gldm_render_depth in
csrc/mesh_render.hip; pointcloud.sample_mesh_surface / render_depth) on one MI355X.  HIP events around warmed calls, medians
of --iterations with min-max, as tools/bench_cluster.py.

  sample    an icosphere of 20480 faces; 1024 and 2^20 points, in-kernel uniforms, through the public entry (allocations and
            the workspace query included)
  render    480 x 640 frames of a table with five such spheres standing on it (102412 triangles per frame), depth + labels +
            faces: one frame, and eight frames from eight poses in one call (per frame); through the public entry, the
            instance table's upload and the read-back of the dropped count included
  numpy     the restatement (tests/mesh_ref.py) at sizes it finishes: 2^16 samples of the same sphere, and one 96 x 128 frame
            of the same scene built from 1280-face spheres; wall clock, one run, each checked bitwise against the entry

    python tools/bench_mesh.py --out profiles/mesh_bench.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from bench_scene import timed  # noqa: E402
from graspldm_amd import mesh as M  # noqa: E402
from graspldm_amd.camera import Camera, look_at  # noqa: E402
from graspldm_amd.pointcloud import render_depth, render_plan, sample_mesh_surface  # noqa: E402

SPOTS = ((-0.3, -0.2), (0.0, 0.25), (0.3, -0.1), (-0.15, 0.05), (0.2, 0.3))


def table_scene(subdivisions, radius=0.08):
    def at(x, y, z):
        m = np.eye(4)
        m[:3, 3] = (x, y, z)
        return m
    meshes = M.MeshBatch([M.box((1.4, 1.4, 0.04)), M.icosphere(subdivisions, radius)])
    inst = [(0, at(0, 0, -0.02), 1)] + [(1, at(x, y, radius), k + 2) for k, (x, y) in enumerate(SPOTS)]
    return meshes, inst


def stats(t):
    return dict(median_ms=t[0], min_ms=t[1], max_ms=t[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import mesh_ref as ref
    res = dict(device=torch.cuda.get_device_name(0))

    sphere = M.MeshBatch([M.icosphere(5, 0.1)])
    sphere.on("cuda")
    for n in (1024, 1 << 20):
        res[f"sample_{n}"] = stats(timed(lambda: sample_mesh_surface(sphere, n, seed=1, return_faces=True), args.iterations,
                                         args.warmup))
    n = 1 << 16
    t0 = time.perf_counter()
    exp = ref.sample_surface(sphere.vertices, sphere.faces, sphere.vert_start, sphere.vert_count, sphere.face_start,
                             sphere.face_count, n, seed=1)
    res["numpy_sample_65536_ms"] = 1e3 * (time.perf_counter() - t0)
    pts, face = sample_mesh_surface(sphere, n, seed=1, return_faces=True)
    assert pts.cpu().numpy().tobytes() == exp["points"].tobytes() and np.array_equal(face.cpu().numpy(), exp["face"])

    cam = Camera.from_intrinsics(600.0, 600.0, 319.5, 239.5, 640, 480)
    meshes, inst = table_scene(5)
    meshes.on("cuda")
    pose = look_at((0.0, -1.0, 0.9), (0, 0, 0))
    res["triangles_per_frame"] = int(render_plan(meshes, cam, pose, [inst])["n_tris"])
    res["render_1_frame"] = stats(timed(lambda: render_depth(meshes, cam, pose, [inst], return_labels=True, return_faces=True),
                                        args.iterations, args.warmup))
    eyes = np.random.default_rng(0).normal(size=(8, 3))
    eyes[:, 2] = np.abs(eyes[:, 2]) + 0.5   # above the table
    poses = np.stack([look_at(1.3 * e / np.linalg.norm(e), (0, 0, 0)) for e in eyes])
    t = timed(lambda: render_depth(meshes, cam, poses, [inst] * 8, return_labels=True, return_faces=True), args.iterations,
              args.warmup)
    res["render_8_frames_per_frame"] = stats(tuple(v / 8 for v in t))
    depth = render_depth(meshes, cam, pose, [inst])
    res["covered_pixels"] = int((depth > 0).sum())

    small_cam = Camera.from_intrinsics(120.0, 120.0, 63.5, 47.5, 128, 96)
    small, inst = table_scene(3)
    plan = render_plan(small, small_cam, pose, [inst])
    t0 = time.perf_counter()
    exp = ref.render(*ref.render_plan_arrays(small, plan))
    res["numpy_render_96x128_6412_triangles_ms"] = 1e3 * (time.perf_counter() - t0)
    d, lab = render_depth(small, small_cam, pose, [inst], return_labels=True)
    assert d.cpu().numpy().tobytes() == exp["depth"].tobytes() and np.array_equal(lab.cpu().numpy(), exp["label"])
    res["render_96x128_6412_triangles"] = stats(timed(lambda: render_depth(small, small_cam, pose, [inst], return_labels=True),
                                                      args.iterations, args.warmup))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
