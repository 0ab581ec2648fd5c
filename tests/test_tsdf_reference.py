"""CPU: the float64 restatement of TSDF fusion and marching tetrahedra (tests/tsdf64.py) against analytic answers, and the mesh PLY round trip.  The
GPU tests (tests/test_gpu_tsdf.py) check the kernels against this restatement; these check the restatement itself."""
import numpy as np
import pytest

from webdgs_amd import loaders, synth

import tsdf64 as t64

MASK_CAP = 0.005   # each mask holds at most this share of the voxels

# ---------------------------------------------------------------- the sphere scene
SPHERE_DIMS = (24, 20, 16)
VOXEL = 0.25
RADIUS = 6 * VOXEL
TRUNC = 4 * VOXEL
IMG_W, IMG_H, FY = 64, 48, 61.3
CAM_DISTANCE = 8.0
CENTRE = np.array([0.171, -0.093, 0.058])
# the sphere's centre lies at (12.37, 10.21, 8.43) voxels of the volume: off the lattice, so that voxel centres do not project onto pixel borders by symmetry
ORIGIN = (CENTRE - np.array([12.37, 10.21, 8.43]) * VOXEL).astype(np.float32)
CENTRE_VOXEL = (12, 10, 8)
# ... and the origin of the volume whose voxel CENTRE_VOXEL is centred on it: the cameras' central rays run through its voxel centres (test_central_ray)
ORIGIN_ON_RAY = (CENTRE - (np.array(CENTRE_VOXEL) + 0.5) * VOXEL).astype(np.float32)


def sphere_centre():
    return CENTRE.copy()


ROLL = 0.37   # radians about the viewing direction: an axis-aligned camera would project whole columns of voxel centres onto one pixel coordinate


def look_at(position, target, roll=ROLL):
    """Row-major world -> view matrix of a camera at ``position`` looking at ``target`` (COLMAP axes: +x right, +y down, +z forward), rolled by
    ``roll`` about the viewing direction."""
    f = np.asarray(target, np.float64) - np.asarray(position, np.float64)
    f /= np.linalg.norm(f)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.9 else np.array([0.0, 0.0, 1.0])
    xr = np.cross(up, f)
    xr /= np.linalg.norm(xr)
    yd = np.cross(f, xr)
    xr, yd = np.cos(roll) * xr + np.sin(roll) * yd, np.cos(roll) * yd - np.sin(roll) * xr
    rot = np.stack([xr, yd, f])
    view = np.eye(4)
    view[:3, :3] = rot
    view[:3, 3] = -rot @ np.asarray(position, np.float64)
    return view


def sphere_cameras():
    """Six 68-float blocks: cameras on the +-axes through the sphere's centre, CAM_DISTANCE away, looking at it."""
    m = sphere_centre()
    cams = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            p = m.copy()
            p[axis] += sign * CAM_DISTANCE
            cams.append(synth.camera_block(look_at(p, m), IMG_W, IMG_H, FY))
    return np.stack(cams)


def sphere_depth(camera):
    """(depth f32 [H, W], weight sum f32 [H, W], rgba8 [H, W, 4]) of the sphere seen from a camera of ``sphere_cameras``: the ray through each pixel
    centre against the sphere (0 where it misses), 1 / 0, and a colour that varies over the image."""
    blk = np.asarray(camera, np.float32).astype(np.float64)
    i, j = np.meshgrid(np.arange(IMG_W) + 0.5, np.arange(IMG_H) + 0.5)
    a = (2.0 * i / IMG_W - 1.0) / blk[32]
    b = (1.0 - 2.0 * j / IMG_H) / blk[37]
    q = a * a + b * b + 1.0
    disc = CAM_DISTANCE ** 2 - q * (CAM_DISTANCE ** 2 - RADIUS ** 2)
    hit = disc >= 0
    z = np.where(hit, (CAM_DISTANCE - np.sqrt(np.where(hit, disc, 0.0))) / q, 0.0)
    colour = np.zeros((IMG_H, IMG_W, 4), np.uint8)
    colour[..., 0] = (np.arange(IMG_W) * 4)[None, :]
    colour[..., 1] = (np.arange(IMG_H) * 5)[:, None]
    colour[..., 2] = 77
    colour[..., 3] = 255
    return z.astype(np.float32), hit.astype(np.float32), colour


def fuse_sphere64(dims=SPHERE_DIMS, views=None, colour=True, origin=ORIGIN):
    """The sphere scene fused in float64: (volume A, volume B, per-view reports)."""
    cams = sphere_cameras()
    va = t64.Volume64(origin, VOXEL, dims, TRUNC, colour=colour)
    vb = va.copy()
    reports = []
    for v in (range(6) if views is None else views):
        d, ws, col = sphere_depth(cams[v])
        reports.append(t64.integrate64(va, vb, d, cams[v], IMG_W, IMG_H, weight_sum=ws, colour=col if colour else None))
    return va, vb, reports


def union_masks(reports):
    return {k: np.any([r[k] for r in reports], axis=0) for k in ("near_edge", "near_cut", "near_zero_z")}


def analytic_sphere_volume(dims, centre=None, radius=RADIUS):
    """(tsdf f32 [nz, ny, nx], weight f32): clamp((|c - m| - r) / truncation, -1, 1) at the float32 voxel centres' float64 positions, weight 1."""
    vol = t64.Volume64(ORIGIN, VOXEL, dims, TRUNC)
    x, y, z = t64._grid(vol.centres64())
    m = sphere_centre() if centre is None else centre
    dist = np.sqrt((x - m[0]) ** 2 + (y - m[1]) ** 2 + (z - m[2]) ** 2)
    return np.clip((dist - radius) / TRUNC, -1.0, 1.0).astype(np.float32), np.ones(dist.shape, np.float32)


def assert_closed_sphere_mesh(keys, positions, centre, radius, what):
    """The assertions on a mesh of the analytic sphere: closed, consistently oriented, genus 0, outward, within half a voxel diagonal of the sphere (a
    linear interpolant of a 1-Lipschitz field over one lattice edge of length <= sqrt(3) voxel: the zero of the interpolant is within half the edge of
    a true zero)."""
    verts, faces = t64.weld(keys, positions)
    topo = t64.mesh_topology(faces)
    assert topo["F"] > 100, f"{what}: {topo}"
    assert topo["closed"], f"{what}: an edge that is not in exactly two triangles"
    assert topo["consistent"], f"{what}: an edge run through twice in one direction"
    assert topo["V"] - topo["E"] + topo["F"] == 2, f"{what}: Euler characteristic {topo['V'] - topo['E'] + topo['F']}"
    P = np.asarray(positions, np.float64)
    normal = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    assert np.all(np.einsum("ij,ij->i", normal, P.mean(axis=1) - centre) > 0), f"{what}: a triangle that faces inward"
    off = np.abs(np.linalg.norm(verts.astype(np.float64) - centre, axis=1) - radius)
    assert off.max() <= 0.5 * np.sqrt(3.0) * VOXEL, f"{what}: a vertex {off.max() / VOXEL:.3f} voxels off the sphere"
    return topo


# ---------------------------------------------------------------- integrate
def test_one_voxel_one_view_by_hand():
    """Identity camera, 4 x 4 image, fy = 2 (P00 = 1, -P11 = 1), a 2^3 volume with centres at x, y = +-0.5, z = 3.5, 4.5, truncation 2, depth 4
    everywhere: t = (4 - 3.5) / 2 = 0.25 in front, (4 - 4.5) / 2 = -0.25 behind; a second view with depth 5: (0.25 + 0.75) / 2 and (-0.25 + 0.25) / 2."""
    cam = synth.camera_block(np.eye(4), 4, 4, 2.0)
    assert cam[32] == 1.0 and cam[37] == -1.0
    va = t64.Volume64((-1, -1, 3), 1.0, (2, 2, 2), 2.0, colour=True)
    vb = va.copy()
    col = np.zeros((4, 4, 4), np.uint8)
    col[..., 0] = 255
    col[..., 1] = 51
    r = t64.integrate64(va, vb, np.full((4, 4), 4.0, np.float32), cam, 4, 4, colour=col)
    assert np.all(r["updated_a"]) and np.all(r["updated_b"])
    assert np.array_equal(va.T[0], np.full((2, 2), 0.25)) and np.array_equal(va.T[1], np.full((2, 2), -0.25))
    assert np.all(va.W == 1) and np.all(va.rgb[0] == 1.0) and np.allclose(va.rgb[1], 0.2, atol=1e-15) and np.all(va.rgb[2] == 0)
    t64.integrate64(va, vb, np.full((4, 4), 5.0, np.float32), cam, 4, 4)
    assert np.array_equal(va.T[0], np.full((2, 2), 0.5)) and np.array_equal(va.T[1], np.full((2, 2), 0.0))
    assert np.all(va.W == 2) and np.array_equal(va.T, vb.T)
    # px = ((0.5 / 3.5) / 2 + 0.5) 4 = 2.2857: pixel 2; a depth image that is valid only there updates only x = +0.5, y = +0.5 of the front layer
    d = np.zeros((4, 4), np.float32)
    d[2, 2] = 4.0
    vc = t64.Volume64((-1, -1, 3), 1.0, (2, 2, 2), 2.0, colour=False)
    r = t64.integrate64(vc, None, d, cam, 4, 4)
    assert r["updated_a"].sum() == 2 and r["updated_a"][0, 1, 1] and r["updated_a"][1, 1, 1]
    # a voxel further behind the surface than the truncation is skipped, one in front by more is clamped to 1
    vd = t64.Volume64((-1, -1, 0), 1.0, (2, 2, 8), 2.0, colour=False)
    r = t64.integrate64(vd, None, np.full((4, 4), 4.0, np.float32), cam, 4, 4)
    assert np.all(vd.T[1] == 1.0) and np.all(vd.W[1] == 1)          # z = 1.5: sdf 2.5, clamped
    assert vd.W[0].sum() == 1 and vd.W[0, 0, 0] == 1                # z = 0.5: px = 0 for x = -0.5 (inside), 4 for x = +0.5 (outside)
    assert np.all(vd.W[6] == 0) and np.all(vd.T[6] == 1.0)          # z = 6.5: sdf -2.5 < -2, skipped
    assert np.all(vd.W[5] == 1) and np.all(vd.T[5] == -0.75)        # z = 5.5: sdf -1.5


@pytest.mark.parametrize("view", range(6))
def test_central_ray(view):
    """One view fused into a fresh volume: along the camera's central ray -- the voxels of the row through the sphere's centre -- T is (d - z) /
    truncation clamped at 1, d the depth of the central pixels, and voxels more than a truncation behind the surface are untouched."""
    cams = sphere_cameras()
    va, vb, _ = fuse_sphere64(views=[view], origin=ORIGIN_ON_RAY)
    d, _, _ = sphere_depth(cams[view])
    centre4 = d[IMG_H // 2 - 1:IMG_H // 2 + 1, IMG_W // 2 - 1:IMG_W // 2 + 1]
    assert np.ptp(centre4) < 1e-6 and abs(float(centre4[0, 0]) - (CAM_DISTANCE - RADIUS)) < 3e-3   # (half a pixel off the axis)
    axis, sign = view // 2, (1.0, -1.0)[view % 2]
    n = SPHERE_DIMS[axis]
    idx = [np.full(n, CENTRE_VOXEL[a]) for a in range(3)]
    idx[axis] = np.arange(n)
    z = CAM_DISTANCE - sign * (np.arange(n) - CENTRE_VOXEL[axis]) * VOXEL   # view-space depth of the row's voxel centres
    sdf = float(centre4[0, 0]) - z
    got_T, got_W = va.T[idx[2], idx[1], idx[0]], va.W[idx[2], idx[1], idx[0]]
    seen = sdf >= -TRUNC + 1e-6
    assert np.array_equal(got_W, seen.astype(np.float64))
    assert np.abs(got_T[seen] - np.minimum(sdf[seen] / TRUNC, 1.0)).max() < 1e-5
    assert np.all(got_T[~seen] == 1.0)
    assert seen.sum() >= 5 and (~seen).sum() >= 2 and (got_T[seen] < 0).any() and (axis != 0 or (got_T[seen] == 1.0).any())   # (only the long axis reaches the clamp)


def test_masks_are_small_and_decisions_agree_outside_them():
    """On the six-view scene each mask holds at most 0.5 % of the voxels (the cap the GPU tests use), and outside the masks the float32 and the float64
    decisions are the same -- which is what the masks are for."""
    for dims in (SPHERE_DIMS, (33, 17, 9)):
        va, vb, reports = fuse_sphere64(dims)
        masks = union_masks(reports)
        share = {k: float(m.mean()) for k, m in masks.items()}
        dist_px, dist_sdf = max(r["dist_px"] for r in reports), max(r["dist_sdf"] for r in reports)
        print(f"tsdf masks {dims}: {share}; largest |f32 - f64|: px / W, py / H {dist_px:.3e}, sdf / truncation {dist_sdf:.3e}")
        assert all(s <= MASK_CAP for s in share.values()), share
        assert 8 * dist_px <= t64.EPS_PIXEL and 8 * dist_sdf <= t64.EPS_SDF
        masked = np.any(list(masks.values()), axis=0)
        for r in reports:
            assert np.array_equal(r["updated_a"][~masked], r["updated_b"][~masked])
        assert np.array_equal(va.W[~masked], vb.W[~masked])
        assert np.abs(va.T - vb.T)[~masked].max() == 0.0
        assert (va.W > 0).mean() > 0.3 and va.W.max() >= 4 and (va.W == 0).any()


def test_fused_sphere_mesh_is_near_the_sphere():
    """The mesh of the six fused views of the sphere lies near the sphere."""
    va, _, _ = fuse_sphere64()
    m = t64.mesh64(va.T.astype(np.float32), va.W.astype(np.float32), ORIGIN, VOXEL)
    verts, faces = t64.weld(m["keys"], m["positions"])
    off = np.abs(np.linalg.norm(verts - sphere_centre(), axis=1) - RADIUS)
    assert faces.shape[0] > 500 and off.max() < 1.5 * VOXEL


# ---------------------------------------------------------------- marching tetrahedra
def test_tetrahedra_tile_the_cell_and_cases_count():
    vol = 0.0
    for t in range(6):
        p = [t64._corner_xyz(c) for c in t64.tet_corners(t)]
        det = np.linalg.det(np.stack([p[1] - p[0], p[2] - p[0], p[3] - p[0]]))
        assert abs(abs(det) - 1.0) < 1e-12
        vol += abs(det) / 6.0
    assert abs(vol - 1.0) < 1e-12
    for t in range(6):
        for mask in range(16):
            inside = tuple(bool(mask >> v & 1) for v in range(4))
            tris = t64.tet_triangles(t, inside)
            assert len(tris) == [0, 1, 2, 1, 0][sum(inside)]
            for tri in tris:
                for u, v in tri:
                    assert inside[t64.tet_corners(t).index(u)] != inside[t64.tet_corners(t).index(v)]   # every vertex on an edge that changes sign
                    assert (u & v) == min(u, v) and 1 <= (u ^ v) <= 7                                     # ... whose key offset exists


@pytest.mark.parametrize("dims,shift", [(SPHERE_DIMS, (0.0, 0.0, 0.0)), (SPHERE_DIMS, (0.07, -0.11, 0.05)), ((33, 17, 9), (0.9, -0.6, -0.45))])
def test_analytic_sphere_mesh_is_closed(dims, shift):
    """A volume written directly with the analytic field of a sphere gives a closed, outward, genus-0 mesh near the sphere (the third case: a smaller
    sphere in the flat volume, off every symmetry)."""
    radius = RADIUS if dims == SPHERE_DIMS else 2.9 * VOXEL
    vol = t64.Volume64(ORIGIN, VOXEL, dims, TRUNC)
    centre = (ORIGIN.astype(np.float64) + 0.5 * np.array(dims) * VOXEL) + np.array(shift) * VOXEL
    x, y, z = t64._grid(vol.centres64())
    T = np.clip((np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius) / TRUNC, -1, 1).astype(np.float32)
    assert T.min() < 0 and T[0].min() > 0 and T[-1].min() > 0 and T[:, 0].min() > 0 and T[:, -1].min() > 0 and T[:, :, 0].min() > 0 and T[:, :, -1].min() > 0
    m = t64.mesh64(T, np.ones(T.shape, np.float32), ORIGIN, VOXEL)
    topo = assert_closed_sphere_mesh(m["keys"], m["positions"], centre, radius, f"{dims} {shift}")
    print(f"analytic sphere {dims} {shift}: {topo}")
    # equal keys carry equal positions
    flat_k, flat_p = m["keys"].reshape(-1), m["positions"].reshape(-1, 3)
    order = np.argsort(flat_k, kind="stable")
    same = flat_k[order][1:] == flat_k[order][:-1]
    assert np.array_equal(flat_p[order][1:][same], flat_p[order][:-1][same])


def test_zero_is_outside_and_invalid_cells_are_left_out():
    """A layer of T == 0 between a negative and a positive half: 0 counts as outside, so the surface runs through the layer's voxel centres (every
    vertex at weight T_A / (T_A - 0) = 1 from the negative corner) and no triangle lies between the layer and the positive half.  A voxel of weight 0
    removes the cells around it: here the four of them that hold the surface."""
    T = np.ones((6, 5, 4), np.float32)
    T[:2] = -1.0
    T[2] = 0.0
    W = np.ones(T.shape, np.float32)
    m = t64.mesh64(T, W, (0, 0, 0), 1.0)
    assert np.all(m["positions"][..., 2] == 2.5)
    area = np.linalg.norm(np.cross(m["positions"][:, 1] - m["positions"][:, 0], m["positions"][:, 2] - m["positions"][:, 0]), axis=1)
    assert (area == 0).any() and (area > 0).any()
    assert np.isclose(area.sum() / 2.0, (5 - 1) * (4 - 1))   # the plane's area over the cells, each covered once
    W[2, 2, 2] = 0.0
    m2 = t64.mesh64(T, W, (0, 0, 0), 1.0)
    assert m2["keys"].shape[0] < m["keys"].shape[0]
    area2 = np.linalg.norm(np.cross(m2["positions"][:, 1] - m2["positions"][:, 0], m2["positions"][:, 2] - m2["positions"][:, 0]), axis=1)
    assert np.isclose(area2.sum() / 2.0, (5 - 1) * (4 - 1) - 4)


# ---------------------------------------------------------------- PLY
@pytest.mark.parametrize("coloured", [True, False])
def test_mesh_ply_round_trip(tmp_path, coloured):
    T, W = analytic_sphere_volume(SPHERE_DIMS)
    m = t64.mesh64(T, W, ORIGIN, VOXEL)
    verts, faces = t64.weld(m["keys"], m["positions"])
    rng = np.random.default_rng(3)
    mesh = dict(vertices=verts.astype(np.float32), faces=faces.astype(np.uint32), colours=rng.integers(0, 256, (verts.shape[0], 3)).astype(np.uint8) if coloured else None)
    path = str(tmp_path / "mesh.ply")
    loaders.saveMeshPLY(path, mesh)
    data = open(path, "rb").read()
    head = data[:data.index(b"end_header\n")].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {verts.shape[0]}"]
    assert ("property uchar red" in head) == coloured and "property list uchar uint vertex_indices" in head
    back = loaders.loadMeshPLY(path)
    assert back["vertices"].tobytes() == mesh["vertices"].tobytes() and back["faces"].tobytes() == mesh["faces"].tobytes()
    assert (back["colours"] is None) == (not coloured) and (not coloured or back["colours"].tobytes() == mesh["colours"].tobytes())
    assert loaders.meshPLYBytes(back) == data
    empty = dict(vertices=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.uint32), colours=None)
    loaders.saveMeshPLY(path, empty)
    assert loaders.loadMeshPLY(path)["faces"].shape == (0, 3)
