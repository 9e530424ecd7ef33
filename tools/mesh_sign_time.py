#!/usr/bin/env python
"""Time of the signed distance to a mesh (thr3ed_atom_amd.mesh_sign: rf_mesh_face_pseudonormals, rf_mesh_signed_distance) on the pair of
tools/mesh_distance_time.py: the raw ``extract_mesh`` surface of the 256^3 sparse scene of tests.helpers.sparse_scene_grid (iso level 5)
and its ``simplify_mesh`` at two voxels, 10^6 area-weighted surface samples of each against the other.  The scene is synthetic and
generated here.  HIP events on one device, two warm-up runs, then N timed runs per step, median / min / max ms:

    tables       mesh_topology (torch) and pseudonormal_tables (one launch and the gather) of each mesh
    sign         the launch of rf_mesh_signed_distance on the forward's faces, with and without the optional outputs, beside the
                 forward query it follows and beside the same rule written in torch gather ops
    volume       mesh_to_sdf of the simplified mesh: 256^3 truncated at 3 voxels (and the share of known nodes), 128^3 exact -- one run
                 each after a small warm-up volume
    direction    the signed mean of simplify_mesh at two voxels with placement "quadric" and "mean" against the raw surface

Writes profiles/mesh_sign_time.json.

    python tools/mesh_sign_time.py [timed runs] [output json]"""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thr3ed_atom_amd as rf  # noqa: E402
from tests.helpers import sparse_scene_grid  # noqa: E402
from thr3ed_atom_amd import mesh_sign  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mesh_sign_time.json")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
G, ISO, SAMPLES = 256, 5.0, 1_000_000
VOXEL = 3.0 / G


def timed(fn, runs=None, warm=2):
    """(median, min, max) ms over `runs` runs after `warm` warm-ups, and the last result"""
    for _ in range(warm):
        result = fn()
    times = []
    for _ in range(reps if runs is None else runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        result = fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return [round(times[len(times) // 2], 4), round(times[0], 4), round(times[-1], 4)], result


def say(report, key):
    print(json.dumps({key: report[key]}), flush=True)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def unit(a, b, c):
    n = torch.linalg.cross(b - a, c - a)
    nn = dot(n, n)
    return torch.where((nn > 0)[:, None], n / torch.sqrt(nn)[:, None], torch.zeros_like(n))


def torch_sign(grid, points, face):
    """the rule of csrc/mesh_sign.h in float32 torch gather ops: what a user without the kernel would have to write"""
    tri = grid.faces[face]
    a, b, c = grid.vertices[tri[:, 0]], grid.vertices[tri[:, 1]], grid.vertices[tri[:, 2]]
    lo, hi = torch.minimum(torch.minimum(a, b), c), torch.maximum(torch.maximum(a, b), c)
    p = points

    def candidate(q):
        q = torch.minimum(torch.maximum(q, lo), hi)
        d = p - q
        return dot(d, d), q

    def segment(s, e):
        g, w = e - s, p - s
        l = dot(g, g)
        t = torch.where(l > 0, (dot(w, g) / l).clamp(0, 1), torch.zeros_like(l))
        return (*candidate(s + t[:, None] * g), t)

    best, q, t = segment(a, b)
    region = torch.zeros_like(face)
    for k, (s, e) in ((1, (b, c)), (2, (c, a))):
        d2, qk, tk = segment(s, e)
        take = d2 < best
        best, q, t, region = torch.where(take, d2, best), torch.where(take[:, None], qk, q), torch.where(take, tk, t), torch.where(take, k, region)
    n = torch.linalg.cross(b - a, c - a)
    nn = dot(n, n)
    foot = p - (dot(p - a, n) / nn)[:, None] * n
    edge = lambda s, e: dot(torch.linalg.cross(e - s, foot - s), n)  # noqa: E731
    e_ab, e_bc, e_ca = edge(a, b), edge(b, c), edge(c, a)
    d2, qp = candidate(foot)
    take = (nn > 0) & (e_ab >= 0) & (e_bc >= 0) & (e_ca >= 0) & (d2 < best) & ((e_ab + e_bc) + e_ca > 0)
    best, q, region = torch.where(take, d2, best), torch.where(take[:, None], qp, q), torch.where(take, 3, region)
    at_start, at_end = (region < 3) & (1.0 - t == 1.0), (region < 3) & (t == 1.0)
    corner = torch.where(at_start, region, (region + 1) % 3)
    vertex = tri.gather(1, corner.clamp(max=2)[:, None])[:, 0]
    own = unit(a, b, c)
    other = grid_partners[face, region.clamp(max=2)].long()
    mate = grid.faces[other.clamp(min=0)]
    across = unit(grid.vertices[mate[:, 0]], grid.vertices[mate[:, 1]], grid.vertices[mate[:, 2]])
    normal = torch.where((region == 3)[:, None], own, torch.where((at_start | at_end)[:, None], grid_vertex_normals[vertex],
                                                                   torch.where((other >= 0)[:, None], own + across, own)))
    d = torch.sqrt(best)
    return torch.where(dot(p - q, normal) < 0, -d, d)


def main():
    global grid_partners, grid_vertex_normals
    dens, feat = sparse_scene_grid((G, G, G), 27, 11)
    field = rf.VoxelGrid(dens.to(dev), feat.to(dev), rf.VoxelSize(VOXEL, VOXEL, VOXEL), density_preactivation=torch.nn.Identity(),
                         density_postactivation=torch.nn.ReLU(), expected_density_scale=100.0 / 3.0, storage="split")
    report = {"device": torch.cuda.get_device_name(dev), "scene": f"synthetic sparse scene of tests.helpers.sparse_scene_grid at {G}^3, iso level {ISO}, generated in the tool",
              "runs": reps, "columns": "median, min, max ms (HIP events, one device, two warm-up runs)", "samples": SAMPLES}
    warnings.simplefilter("ignore", RuntimeWarning)  # (the simplified mesh is not closed: its own sign is timed, not trusted)
    with torch.no_grad():
        raw = rf.extract_mesh(field, ISO, subdivisions=1)
        raw = rf.Mesh(raw.vertices, raw.faces, None, None)
        small = rf.simplify_mesh(raw, float(np.float32(2 * VOXEL)))
        meshes = {"raw": raw, "simplified": small}
        samples = {name: rf.sample_mesh_surface(mesh, SAMPLES, seed=k)[0] for k, (name, mesh) in enumerate(meshes.items())}
        for name, mesh in meshes.items():
            other = "simplified" if name == "raw" else "raw"
            row = {"V": int(mesh.vertices.shape[0]), "T": int(mesh.faces.shape[0])}
            row["topology_ms"], topology = timed(lambda: rf.mesh_topology(mesh))
            row["topology"] = {k: v for k, v in topology._asdict().items() if k != "partners"}
            row["tables_ms"], _ = timed(lambda: mesh_sign.pseudonormal_tables(mesh.vertices, mesh.faces))
            signs = rf.MeshSignGrid(mesh)
            points = samples[other]
            row["queries"] = f"{SAMPLES} surface samples of the {other} mesh"
            row["forward_closest_call_ms"], found = timed(lambda: signs.grid.closest(points))
            signed = torch.empty(SAMPLES, device=dev)
            feature, normal = torch.empty((SAMPLES, 2), dtype=torch.int32, device=dev), torch.empty((SAMPLES, 3), device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            launch = lambda **kw: mesh_sign.signed_distance_raw(signs.vertices, signs.faces, signs.topology.partners, signs.vertex_normals, points, found.face, signed,  # noqa: E731
                                                                status, **kw)
            row["sign_launch_ms"], _ = timed(lambda: launch())
            row["sign_launch_all_outputs_ms"], _ = timed(lambda: launch(feature=feature, normal=normal))
            row["signed_distance_call_ms"], whole = timed(lambda: signs.signed_distance(points))
            grid_partners, grid_vertex_normals = signs.topology.partners, signs.vertex_normals
            row["torch_gather_rule_ms"], theirs = timed(lambda: torch_sign(signs, points, found.face))
            row["torch_equal_signs"] = float(((theirs < 0) == (signed < 0)).double().mean())
            row["torch_over_launch"] = round(row["torch_gather_rule_ms"][0] / row["sign_launch_ms"][0], 1)
            row["launch_over_forward"] = round(row["sign_launch_ms"][0] / row["forward_closest_call_ms"][0], 4)
            row["feature_kinds_face_edge_vertex"] = torch.bincount(feature[:, 0].long(), minlength=3).cpu().tolist()
            row["inside_share"] = float((whole.distance < 0).double().mean())
            row["status"] = int(status.item())
            report[f"queries_against_{name}"] = row
            say(report, f"queries_against_{name}")
        lo, hi = (-1.5,) * 3, (1.5,) * 3
        rf.mesh_to_sdf(small, lo, hi, (16, 16, 16))
        volume = {}
        ms, cut = timed(lambda: rf.mesh_to_sdf(small, lo, hi, (256,) * 3, truncation=3 * VOXEL), runs=1, warm=0)
        volume["truncated_256_ms"], volume["truncated_256_known_share"] = ms[0], float(cut.known.double().mean())
        report["mesh_to_sdf_of_the_simplified_mesh"] = volume
        say(report, "mesh_to_sdf_of_the_simplified_mesh")
        del cut
        ms, exact = timed(lambda: rf.mesh_to_sdf(small, lo, hi, (128,) * 3), runs=1, warm=0)
        volume["exact_128_ms"], volume["exact_128_inside_share"] = ms[0], float((exact.sdf < 0).double().mean())
        say(report, "mesh_to_sdf_of_the_simplified_mesh")
        direction = {}
        for placement in ("quadric", "mean"):
            simplified = rf.simplify_mesh(raw, float(np.float32(2 * VOXEL)), placement=placement)
            result = rf.signed_mesh_distance(simplified, raw, samples=SAMPLES)
            direction[placement] = {"faces": int(simplified.faces.shape[0]), "signed_mean_in_voxels": result.a_to_b.mean / VOXEL, "inside_share": result.a_to_b.inside,
                                    "mean_inside_in_voxels": result.a_to_b.mean_inside / VOXEL, "mean_outside_in_voxels": result.a_to_b.mean_outside / VOXEL}
        direction["note"] = "samples of the simplified mesh against the raw surface, which is closed: negative = inside the raw surface"
        report["simplified_against_raw"] = direction
        say(report, "simplified_against_raw")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report), flush=True)


if __name__ == "__main__":
    main()
