"""The restatement of the texture atlas (tests/meshtexture_ref.py) against the properties DESIGN.md section 23 claims, without a GPU: a bilinear lookup inside a
face's UV triangle touches only that face's texels, ownership, the texture coordinates, the host's layout, order-independence, the face-level rules on the
crafted mesh, the analytic ramp, and the OBJ round trip."""
import os

import numpy as np
import pytest

from webdgs_amd import loaders, ops

import meshtexture_ref as T


# ---------------------------------------------------------------- the atlas
@pytest.mark.parametrize("C", T.CELLS)
def test_a_bilinear_lookup_inside_a_face_touches_only_its_own_texels(C):
    """Brute force over a dense barycentric grid: the lookup at a point of the chart triangle, in texel-centre coordinates, reads the texels floor and
    floor + 1 on each axis (those with a non-zero weight); each must be in the cell and owned by the face."""
    m, n = C - 3, 96
    for odd in (0, 1):
        for a in range(n + 1):
            for b in range(n + 1 - a):
                u, v = m * a / n, m * b / n   # exact position between the corners (0, 0), (m, 0), (0, m), in texels
                x, y = (C - 1 - u, C - 1 - v) if odd else (u, v)
                for i in {int(np.floor(x)), int(np.ceil(x))}:
                    for j in {int(np.floor(y)), int(np.ceil(y))}:
                        assert 0 <= i < C and 0 <= j < C, "the lookup leaves the cell"
                        assert T.owner(i, j, C) == odd, f"C = {C}: the lookup at ({x}, {y}) touches ({i}, {j}), which the face does not own"


@pytest.mark.parametrize("C", T.CELLS)
def test_every_texel_has_at_most_one_owner_and_the_diagonal_none(C):
    for F in (1, 2, 3, 7, 11, 129):
        L, tx = T.layout(F, C), T.texels(F, C)
        seen = np.zeros((L["height"], L["width"]), np.int64)
        np.add.at(seen, (tx["y"], tx["x"]), 1)
        assert seen.max() == 1
        for k in range(L["cells"]):
            x0, y0 = (k % L["cellsPerRow"]) * C, (k // L["cellsPerRow"]) * C
            for i in range(C):
                assert seen[y0 + C - 1 - i, x0 + i] == 0, "the anti-diagonal is owned"
        per_face = np.bincount(tx["face"], minlength=F)
        assert np.all(per_face == C * (C - 1) // 2), "every face owns a triangle of C (C - 1) / 2 texels"
        assert len(set(tx["row"].tolist())) == tx["row"].shape[0] and tx["row"].max() < L["cells"] * C * C
        assert L["cellsPerRow"] ** 2 >= L["cells"] > (L["cellsPerRow"] - 1) ** 2 and L["rows"] * L["cellsPerRow"] >= L["cells"] > (L["rows"] - 1) * L["cellsPerRow"]


@pytest.mark.parametrize("C", T.CELLS)
def test_texture_coordinates_and_the_hosts_layout(C):
    for F in (0, 1, 2, 3, 7, 11, 129, 1000):
        L, host = T.layout(F, C), ops.textureLayout(F, C)
        assert (host["width"], host["height"], host["cellsPerRow"]) == (L["width"], L["height"], L["cellsPerRow"])
        assert host["uv"].dtype == np.float32 and host["uv"].shape == (F, 3, 2) and host["uv"].tobytes() == L["uv"].tobytes()
        assert np.all((L["uv"] > 0) & (L["uv"] < 1))
        if F:
            # a corner's coordinates are the centre of the texel (i', j') = (0, 0), (m, 0), (0, m) of its face
            tx = T.texels(F, C)
            for c, (ip, jp) in enumerate(((0, 0), (C - 3, 0), (0, C - 3))):
                sel = (tx["ip"] == ip) & (tx["jp"] == jp)
                order = np.argsort(tx["face"][sel])
                x, y = tx["x"][sel][order], tx["y"][sel][order]
                assert np.allclose(L["uv"][:, c, 0] * L["width"] - 0.5, x, atol=1e-3) and np.allclose((1 - L["uv"][:, c, 1]) * L["height"] - 0.5, y, atol=1e-3)
    for bad in ((1, 5), (1, 0), (-1, 8), (2 ** 31, 8), (2 * (16384 // C) ** 2 + 1, C)):
        with pytest.raises(ValueError):
            ops.textureLayout(*bad)
    assert ops.textureLayout(2 * (16384 // C) ** 2, C)["width"] == 16384


# ---------------------------------------------------------------- the definition
def test_three_views_in_two_orders_give_equal_bytes():
    m = T.case(T.THREE_VIEWS)
    a, b = T.run(m, order=(0, 1, 2)), T.run(m, order=(2, 0, 1))
    assert T.digest(a) == T.digest(b) == T.digest(T.expected(T.THREE_VIEWS))
    assert a["rows"].any() and (a["texelState"] == 1).any()


@pytest.mark.parametrize("name", sorted(T.EXPECT))
def test_the_face_totals_the_cases_are_about(name):
    totals = T.expected(name)["totals"]
    for k, v in T.EXPECT[name].items():
        assert totals[k] == v, f"{name}: {k} = {totals[k]}, expected {v}"


def test_the_crafted_geometry_meets_every_rule():
    m = T.case("geometry-cell-8")
    C, F = 8, m["faces"].shape[0]
    tx = T.texels(F, C)
    per_view = []
    for w in m["views"]:
        s = T.new_state(F, C)
        T.accumulate(s, m["vertices"], m["faces"], w["camera"], w["image"], w["depth"], w["width"], w["height"], w["near"], w["depth_tolerance"], w["min_cos"],
                     w["two_sided"])
        touched = np.zeros(F, bool)
        touched[tx["face"][s["rows"][tx["row"], 3] > 0]] = True
        per_view.append(touched)
    occluded, open_, two_sided = per_view
    for f in (0, 1, 6, 7, 8, 9, 10):   # behind near, crossing near, zero area, an index >= V, a NaN vertex, off the image, grazing
        assert not occluded[f] and not open_[f] and not two_sided[f], f"face {f} was coloured"
    assert occluded[2] and occluded[5], "the half-visible face and the front face are coloured"
    assert not occluded[3] and not open_[3] and two_sided[3], "the back-facing face is coloured only two-sided"
    assert not occluded[4] and open_[4], "the hidden face is coloured only without the occlusion test"
    # half outside the image: some of face 2's texels are usable and outside
    assert 0 < int((T.expected("geometry-cell-8")["texelState"] == 1).sum())


def test_resolve_fills_from_one_three_and_no_neighbours():
    m, want = T.case("resolve-colours"), T.expected("resolve-colours")
    C, F = m["cell"], m["faces"].shape[0]
    tx = T.texels(F, C)
    state = want["texelState"]
    baked = np.zeros((T.layout(F, C)["height"] + 2, T.layout(F, C)["width"] + 2), np.int64)
    owner = np.full(baked.shape, -1, np.int64)
    baked[tx["y"] + 1, tx["x"] + 1] = state[tx["y"], tx["x"]] == 1
    owner[tx["y"] + 1, tx["x"] + 1] = tx["face"]
    counts = np.zeros(tx["x"].shape[0], np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                counts += baked[tx["y"] + 1 + dy, tx["x"] + 1 + dx] * (owner[tx["y"] + 1 + dy, tx["x"] + 1 + dx] == tx["face"])
    mine = state[tx["y"], tx["x"]]
    assert np.all((mine == 2) == ((mine != 1) & (counts > 0)))
    filled = set(counts[mine == 2].tolist())
    assert {1, 3} <= filled, f"filled from {sorted(filled)} neighbours"
    assert np.any((mine == 0) & (counts == 0))
    # without colours the fallback is black and opaque; with them it is not
    none = T.expected("resolve-no-colours")
    assert np.all(none["texture"][tx["y"], tx["x"]][mine == 0] == np.array([0, 0, 0, 255], np.uint8))
    assert want["texture"][tx["y"], tx["x"]][mine == 0][:, :3].any()
    # min_weight above and below the sums
    assert 0 < T.expected("resolve-min-weight-300")["totals"]["bakedTexels"] < want["totals"]["bakedTexels"]
    assert T.expected("resolve-min-weight-600")["totals"]["bakedTexels"] == 0
    # nobody's texels are zero
    nobody = np.ones(state.shape, bool)
    nobody[tx["y"], tx["x"]] = False
    assert not want["texture"][nobody].any() and not state[nobody].any()


@pytest.mark.parametrize("C", T.CELLS)
def test_the_ramp_is_reproduced_within_two_levels(C):
    """The bound: the snap moves the sample by at most 1/512 pixel on each axis, at most 2/512 level under slopes of at most one level a pixel; the
    photograph's quantisation at most 0.5; the sample's rounding to a byte at most 0.5; the mean's rounding at most 0.5: below 2."""
    scene = T.analytic_scene(C)
    out = T.run(scene["case"])
    errors, n = T.analytic_errors(scene, out["texture"], out["texelState"])
    assert n >= 2 * 3, "the interior texels of both faces are baked"
    assert n == 2 * (C - 2) * (C - 1) // 2, "every interior texel of both faces is baked"
    assert errors.max() <= 2.0, f"C = {C}: {errors.max()} levels off the ramp"


# ---------------------------------------------------------------- OBJ
def test_obj_round_trip_is_exact(tmp_path):
    rng = np.random.default_rng(5)
    for normals in (False, True):
        F, V, C = 11, 9, 8
        L = ops.textureLayout(F, C)
        mesh = dict(vertices=rng.normal(0, 3, (V, 3)).astype(np.float32), faces=rng.integers(0, V, (F, 3)).astype(np.uint32), uv=L["uv"],
                    texture=rng.integers(0, 256, (L["height"], L["width"], 4)).astype(np.uint8))
        mesh["vertices"][0] = [1e-30, -3.4e38, 0.1]
        if normals:
            mesh["normals"] = rng.normal(0, 1, (V, 3)).astype(np.float32)
        path = str(tmp_path / f"mesh{int(normals)}.obj")
        loaders.saveMeshOBJ(path, mesh)
        assert sorted(os.listdir(tmp_path))[-3:] == [f"mesh{int(normals)}.mtl", f"mesh{int(normals)}.obj", f"mesh{int(normals)}.png"]
        back = loaders.loadMeshOBJ(path)
        assert set(back) == set(mesh)
        for k in mesh:
            assert back[k].dtype == mesh[k].dtype and back[k].shape == mesh[k].shape and back[k].tobytes() == mesh[k].tobytes(), k
        text = open(path).read()
        assert text.count("\nvt ") == 3 * F and text.count("\nf ") == F and "usemtl" in text
    with pytest.raises(ValueError):
        loaders.saveMeshOBJ(str(tmp_path / "mesh.ply"), mesh)


def test_the_node_hosts_obj_files_are_the_python_hosts(tmp_path):
    """bindings/ts/loaders.js needs no device: the same mesh written by both hosts gives the same three files, ties of "%.9g" included."""
    import json
    import shutil
    import subprocess
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(3)
    F, V, C = 11, 40, 8
    L = ops.textureLayout(F, C)
    v = (rng.normal(0, 3, (V, 3)) * 10.0 ** rng.integers(-8, 8, (V, 1))).astype(np.float32)
    v[0] = [0.5009765625, -0.0, 1e-30]          # a tie at the tenth digit, a negative zero, a small exponent
    v[1] = [-3.4e38, 123456792.0, 0.0001]
    v[2] = [99999.9999, 0.00001, 1.5]
    v[3] = [16777216.0, 999999999.0, 0.000099999997]
    mesh = dict(vertices=v, faces=rng.integers(0, V, (F, 3)).astype(np.uint32), uv=L["uv"], texture=rng.integers(0, 256, (L["height"], L["width"], 4)).astype(np.uint8),
                normals=rng.normal(0, 1, (V, 3)).astype(np.float32))
    for host in ("py", "js"):
        os.makedirs(tmp_path / host)
    loaders.saveMeshOBJ(str(tmp_path / "py" / "mesh.obj"), mesh)
    for k, a in mesh.items():
        a.tofile(str(tmp_path / f"{k}.bin"))
    script = """
const fs = require('fs'), path = require('path'), L = require(process.argv[1]), dir = process.argv[2], m = JSON.parse(process.argv[3]);
const rd = (n, T) => { const b = fs.readFileSync(path.join(dir, n + '.bin')); return new T(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const mesh = { vertices: rd('vertices', Float32Array), faces: rd('faces', Uint32Array), uv: rd('uv', Float32Array), texture: rd('texture', Uint8Array),
  normals: rd('normals', Float32Array), textureWidth: m.w, textureHeight: m.h };
L.saveMeshOBJ(path.join(dir, 'js', 'mesh.obj'), mesh);
const back = L.loadMeshOBJ(path.join(dir, 'js', 'mesh.obj'));
for (const k of ['vertices', 'faces', 'uv', 'texture', 'normals'])
  if (!Buffer.from(back[k].buffer, back[k].byteOffset, back[k].byteLength).equals(Buffer.from(mesh[k].buffer, mesh[k].byteOffset, mesh[k].byteLength))) throw new Error(k);
console.log('OBJ_OK');
"""
    r = subprocess.run([node, "-e", script, os.path.join(root, "bindings", "ts", "loaders.js"), str(tmp_path), json.dumps(dict(w=L["width"], h=L["height"]))],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OBJ_OK" in r.stdout, r.stderr[-2000:]
    for name in ("mesh.obj", "mesh.mtl", "mesh.png"):
        assert (tmp_path / "js" / name).read_bytes() == (tmp_path / "py" / name).read_bytes(), name
