"""The closed-form per-triangle atlas, its bake kernel and the textured-mesh export (tssplat_amd/atlas.py, csrc/texture_*,
MeshRasterizer.export) against tests/atlas_oracle.py.  CPU: layout, tap ownership, writer / loader.  GPU: the bake on four
shapes, an out-of-range index, and the closed loop field -> bake -> dr.texture -> export -> load -> render."""
import os

import numpy as np
import pytest

import atlas_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mario():
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    return m["vertices"].astype(np.float32), m["faces"].astype(np.int32)


def _icosahedron():
    g = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float32)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], np.int32)
    return v, f


# ---------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("T", [1, 2, 3, 20, 7409])
@pytest.mark.parametrize("R", [6, 64, 70, 512])
def test_layout_matches_the_oracle(T, R):
    from tssplat_amd import atlas
    try:
        want = AO.layout(T, R)
    except ValueError as e:
        with pytest.raises(ValueError, match=" is " + str(e).split(": ")[1] + "$"):      # the same smallest workable resolution
            atlas.atlas_layout(T, R)
        return
    assert atlas.atlas_layout(T, R) == want
    n, c, L = want
    assert n * n >= (T + 1) // 2 and c * n <= R < (c + 1) * n and L == c - 5 >= 1


@pytest.mark.parametrize("T,R,smallest", [(3, 11, 12), (7409, 256, 366)])
def test_too_small_a_texture_names_the_smallest_workable_one(T, R, smallest):
    from tssplat_amd import atlas
    with pytest.raises(ValueError, match=f" is {smallest}$"):
        atlas.atlas_layout(T, R)
    with pytest.raises(ValueError, match=f" is {smallest}$"):
        atlas.atlas_uv(T, R)
    assert atlas.atlas_layout(T, smallest)[1] == 6 and atlas.atlas_layout(T, smallest)[2] == 1
    with pytest.raises(ValueError):
        atlas.atlas_layout(T, smallest - 1)


def test_uv_matches_the_oracle_and_is_per_wedge():
    from tssplat_amd import atlas
    for T, R in [(1, 6), (3, 12), (20, 70), (7409, 512)]:
        uv, uv_idx = atlas.atlas_uv(T, R)
        want_uv, want_idx = AO.uv(T, R)
        assert uv.dtype.is_floating_point and uv.numpy().dtype == np.float32 and uv_idx.numpy().dtype == np.int32
        assert uv.shape == (3 * T, 2) and uv_idx.shape == (T, 3)
        assert np.array_equal(uv.numpy(), want_uv.astype(np.float32)) and np.array_equal(uv_idx.numpy(), want_idx)
        corners = want_uv.reshape(T, 3, 2)                                   # both halves keep the orientation (positive area)
        e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
        assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()
        texel = want_uv * R                                                  # every corner is a texel centre
        assert np.allclose(texel - 0.5, np.round(texel - 0.5), atol=1e-9)


@pytest.mark.parametrize("T,R", [(20, 64), (7409, 512)])
def test_every_bilinear_tap_of_a_triangle_is_a_texel_it_owns(T, R):
    """Random points, all corners, edge points and lattice points of every UV triangle: each tap of non-zero weight is owned by
    the triangle (T = 7409, R = 512: c = 8, L = 3, the smallest leg in use).  R is a power of two, so the float32 uv times R are
    the exact texel coordinates, and the edge and lattice points are built without a rounding: a point of the hypotenuse with
    two integer coordinates has ONE tap, and must not be given a second one by noise in the test's own arithmetic."""
    from tssplat_amd import atlas
    uv, uv_idx = atlas.atlas_uv(T, R)
    L = AO.layout(T, R)[2]
    owner, _, _ = AO.texel_tables(T, R)
    corners = uv.numpy().astype(np.float64)[uv_idx.numpy().astype(np.int64)] * R        # [T, 3, 2] texel coordinates, exact
    assert np.array_equal(corners * 2, np.round(corners * 2))
    d1, d2 = (corners[:, 1] - corners[:, 0]) / L, (corners[:, 2] - corners[:, 0]) / L    # one texel along each leg: 0, +-1
    assert set(np.unique(np.abs(np.concatenate([d1, d2])))) == {0.0, 1.0}
    pts = []
    for m in range(4 * L + 1):                                                          # the three edges in quarter texels
        pts += [corners[:, 0] + d1 * (m / 4), corners[:, 0] + d2 * (m / 4), corners[:, 1] + (d2 - d1) * (m / 4)]
    for a in range(L + 1):                                                              # lattice points (texel centres)
        pts += [corners[:, 0] + d1 * a + d2 * b for b in range(L + 1 - a)]
    rng = np.random.default_rng(7)
    r = rng.random((64, 2))                                                             # interior points
    r = np.where(r.sum(1, keepdims=True) > 1, 1 - r, r) * L
    pts += [corners[:, 0] + d1 * ra + d2 * rb for ra, rb in r]
    pts = np.stack(pts, 1) / R                                                          # [T, P, 2] uv
    tri_of = np.broadcast_to(np.arange(T)[:, None], pts.shape[:2])
    checked = 0
    for i, j, w in AO.bilinear_taps(pts[..., 0], pts[..., 1], R):
        used = w != 0
        assert (i[used] >= 0).all() and (i[used] < R).all() and (j[used] >= 0).all() and (j[used] < R).all()
        assert np.array_equal(owner[j[used], i[used]], tri_of[used])
        checked += int(used.sum())
    assert checked >= T * pts.shape[1]


def test_owner_image_properties():
    for T, R in [(1, 6), (3, 12), (20, 70)]:
        n, c, L = AO.layout(T, R)
        owner, b1, b2 = AO.texel_tables(T, R)
        assert owner.max() == T - 1 and (owner[n * c:] == -1).all() and (owner[:, n * c:] == -1).all()
        counts = np.bincount(owner[owner >= 0], minlength=T)
        assert (counts == c * (c - 1) // 2).all()                        # two halves and one unowned diagonal per cell


def test_writer_and_loader_round_trip(tmp_path):
    from tssplat_amd import atlas
    rng = np.random.default_rng(3)
    T, R = 3, 12
    v = rng.normal(size=(5, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 3]], np.int32)
    uv, uv_idx = atlas.atlas_uv(T, R)
    tex = rng.uniform(-0.2, 1.2, size=(R, R, 3)).astype(np.float32)
    tex[0, 0], tex[0, 1], tex[1, 0] = (0.0, 0.5, 1.0), (0.25, 0.75, 2.0), (0.4980392, 0.5019608, -1.0)
    atlas.write_textured_obj(str(tmp_path), "thing", v, f, uv, uv_idx, tex)
    assert sorted(os.listdir(tmp_path)) == ["thing.mtl", "thing.obj", "thing.png"]

    # the PNG: 8-bit RGB, round(clamp(c, 0, 1) * 255), image rows top-down = texel rows R - 1 ... 0
    want = np.rint(np.clip(tex.astype(np.float64), 0, 1) * 255).astype(np.uint8)[::-1]
    data = open(tmp_path / "thing.png", "rb").read()
    assert np.array_equal(atlas.decode_png_rgb8(data), want)
    assert want[-1, 0].tolist() == [0, 128, 255] and want[-1, 1].tolist() == [64, 191, 255] and want[-2, 0].tolist() == [127, 128, 0]
    try:                                                                  # an independent decoder, where there is one
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(tmp_path / "thing.png") as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), want)

    # the OBJ: 1-based, per-wedge
    lines = open(tmp_path / "thing.obj").read().splitlines()
    assert "mtllib thing.mtl" in lines and "usemtl thing" in lines
    assert sum(ln.startswith("v ") for ln in lines) == 5 and sum(ln.startswith("vt ") for ln in lines) == 3 * T
    faces = [ln for ln in lines if ln.startswith("f ")]
    assert faces == ["f 1/1 2/2 3/3", "f 3/4 2/5 4/6", "f 5/7 1/8 4/9"]
    assert "map_Kd thing.png" in open(tmp_path / "thing.mtl").read().splitlines()

    v2, f2, uv2, idx2, tex2 = atlas.load_textured_obj(str(tmp_path), "thing")
    assert v2.dtype == np.float32 and np.array_equal(v2, v) and f2.dtype == np.int32 and np.array_equal(f2, f)
    assert uv2.dtype == np.float32 and np.array_equal(uv2, uv.numpy()) and np.array_equal(idx2, uv_idx.numpy())
    assert tex2.dtype == np.float32 and tex2.shape == (R, R, 3)
    assert np.array_equal(tex2, want[::-1].astype(np.float32) / np.float32(255))


# ---------------------------------------------------------------------------------------------------------------- GPU, bake

def _bake_case(name):
    rng = np.random.default_rng(11)
    if name == "one":                      # one cell at the minimum size
        return rng.normal(size=(3, 3)).astype(np.float32), np.array([[2, 0, 1]], np.int32), 6
    if name == "three":                    # an odd count: the last half cell is empty
        return rng.normal(size=(5, 3)).astype(np.float32) * 3, np.array([[0, 1, 2], [2, 1, 3], [4, 0, 3]], np.int32), 12
    if name == "icosahedron":              # R is no multiple of c: the trailing texels are unowned
        return _icosahedron() + (70,)
    return _mario() + (512,)


def _check_bake(v, f, R, positions, owner):
    want_p, want_owner, b1, b2 = AO.bake(v, f, R)
    assert owner.dtype == np.int32 and np.array_equal(owner, want_owner)
    # fp32 roundings per component: one per quotient (b1, b2), two in b0 = 1 - b1 - b2, three products and two sums: 8, each
    # at most 2^-24 relative to a term bounded by (1 + |b1| + |b2|) max|v|
    bound = 8 * 2.0 ** -24 * (1 + np.abs(b1) + np.abs(b2)) * np.abs(v).max()
    err = np.abs(positions.astype(np.float64) - want_p).max(axis=-1)
    print(f"bake R={R} T={f.shape[0]}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert (positions[owner < 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "three", "icosahedron", "mario"])
def test_bake_positions_matches_the_oracle(name):
    import torch
    from tssplat_amd import atlas
    v, f, R = _bake_case(name)
    positions, owner = atlas.bake_positions(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), R)
    assert positions.shape == (R, R, 3) and owner.shape == (R, R) and owner.dtype == torch.int32
    assert torch.equal(owner.cpu(), torch.from_numpy(AO.texel_tables(f.shape[0], R)[0]))
    _check_bake(v, f, R, positions.cpu().numpy(), owner.cpu().numpy())


@pytest.mark.gpu
def test_bake_treats_a_triangle_with_an_out_of_range_index_as_unowned():
    import torch
    from tssplat_amd import atlas
    v, f, R = _bake_case("icosahedron")
    clean_p, clean_o = atlas.bake_positions(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), R)
    for bad in (v.shape[0], -1, 2 ** 31 - 1):
        g = f.copy()
        g[7, 1] = bad
        p, o = atlas.bake_positions(torch.from_numpy(v).cuda(), torch.from_numpy(g).cuda(), R)
        hit = clean_o == 7
        assert int(hit.sum()) > 0 and (o[hit] == -1).all() and (p[hit] == 0).all()
        assert torch.equal(o[~hit], clean_o[~hit]) and torch.equal(p[~hit], clean_p[~hit])      # nothing else changes
        _check_bake(v, g, R, p.cpu().numpy(), o.cpu().numpy())


@pytest.mark.gpu
def test_bake_refuses_cpu_tensors_and_small_textures():
    import torch
    from tssplat_amd import atlas
    v, f, R = _bake_case("three")
    with pytest.raises(RuntimeError):
        atlas.bake_positions(torch.from_numpy(v), torch.from_numpy(f), R)
    with pytest.raises(ValueError, match=" is 12$"):
        atlas.bake_positions(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), 11)


# ---------------------------------------------------------------------------------------------------------------- GPU, closed loop

FREQ = (3.0, 4.0, 5.0)


def _field_module():
    import torch

    class Field(torch.nn.Module):
        """The analytic colour field of tools/train_texture.py."""

        def forward(self, positions):
            return {"color": 0.5 + 0.5 * torch.sin(torch.stack([FREQ[0] * positions[..., 0] + 1.0, FREQ[1] * positions[..., 1],
                                                                 FREQ[2] * positions[..., 2] - 0.5], -1))}
    return Field()


@pytest.fixture(scope="module")
def loop():
    """mario, 2 views of scenes.dataset_mvps at 128^2, R = 1024 (c = 16, L = 11): the colour rendered directly, the baked
    texture, and the error budget E of the comparison."""
    import torch
    from tssplat_amd import atlas, dr, geometry, renderers, scenes
    R, res, views = 1024, 128, 2
    v, f = _mario()
    assert atlas.atlas_layout(f.shape[0], R) == (61, 16, 11)
    geo = geometry.TetMeshGeometry(v, np.zeros((0, 4), np.int32), use_smooth_barrier=False, optimize_geo=False,
                                   surface_vid=np.arange(v.shape[0], dtype=np.int32), surface_fid=f)
    field = _field_module()
    ren = renderers.MeshRasterizer(geo, field)
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    v_pos, tri = geo.tet_v, geo.surface_fid
    with torch.no_grad():
        pos_clip = ren.transform_pos(mvp, v_pos).contiguous()
        rast, _ = dr.rasterize(ren.glctx, pos_clip, tri, resolution=[res, res], grad_db=False)
        fg = rast[..., 3] > 0
        direct = field(dr.interpolate(v_pos[None], rast, tri)[0])["color"]
        tex = atlas.bake_material(field, v_pos, tri, R)
        _, owner = atlas.bake_positions(v_pos, tri, R)
    assert int(fg.sum()) > 1000
    # E = k^2 / 8 (h / L)^2 + E32.  First term: bilinear interpolation of 0.5 + 0.5 sin(k x) over one texel, whose sides are at
    # most h / L long in space (h: the longest surface edge, spread over L texels), |second derivative| <= k^2 / 2 along each of
    # the two axes: 2 x (1 / 8) (h / L)^2 k^2 / 2.  E32 = 8 x 2^-24 R G: the fp32 rounding of the interpolated uv (of order 1)
    # and of x = u R - 0.5, a few 2^-24 R texels, times G, the largest texel-to-texel colour step inside a triangle.
    k, L = max(FREQ), 11
    edges = np.concatenate([v[f[:, a]] - v[f[:, b]] for a, b in ((0, 1), (1, 2), (2, 0))])
    h = float(np.sqrt((edges.astype(np.float64) ** 2).sum(1)).max())
    same_x = (owner[:, 1:] == owner[:, :-1]) & (owner[:, 1:] >= 0)
    same_y = (owner[1:] == owner[:-1]) & (owner[1:] >= 0)
    G = max(float((tex[:, 1:] - tex[:, :-1]).abs().amax(-1)[same_x].max()), float((tex[1:] - tex[:-1]).abs().amax(-1)[same_y].max()))
    E = k * k / 8 * (h / L) ** 2 + 8 * 2.0 ** -24 * R * G
    print(f"closed loop: h = {h:.4f}, G = {G:.4f}, E = {E:.5f}, foreground pixels = {int(fg.sum())}")
    return dict(geo=geo, ren=ren, field=field, mvp=mvp, pos_clip=pos_clip, rast=rast, fg=fg, direct=direct, tex=tex, owner=owner, E=E,
                R=R, res=res)


def _render_textured(loop, tex, uv, uv_idx):
    from tssplat_amd import dr
    texc, _ = dr.interpolate(uv[None].contiguous(), loop["rast"], uv_idx)
    return dr.texture(tex[None].contiguous(), texc, filter_mode="linear", boundary_mode="clamp")


@pytest.mark.gpu
def test_baked_texture_renders_the_field(loop):
    import torch
    geo = loop["geo"]
    uv, uv_idx = geo.uv, geo.uv_idx                                      # the atlas at the geometry's default resolution, 1024
    assert uv.is_cuda and uv.shape == (3 * geo.surface_fid.shape[0], 2) and uv_idx.dtype == torch.int32 and geo.uv is uv
    assert (loop["tex"][loop["owner"] < 0] == 0).all()
    with torch.no_grad():
        textured = _render_textured(loop, loop["tex"], uv, uv_idx)
    err = (textured - loop["direct"]).abs()[loop["fg"]]
    print(f"baked vs direct: max err {float(err.max()):.5f}, E = {loop['E']:.5f}")
    assert float(err.max()) <= loop["E"]


@pytest.mark.gpu
def test_export_load_and_render(loop, tmp_path):
    import torch
    from tssplat_amd import atlas
    loop["ren"].export(str(tmp_path), "material")
    out = tmp_path / "material"
    assert sorted(os.listdir(out)) == ["exported_surface.mtl", "exported_surface.obj", "exported_surface.png"]
    v, f, uv, uv_idx, tex = atlas.load_textured_obj(str(out), "exported_surface")
    geo = loop["geo"]
    assert np.array_equal(v, geo.tet_v.cpu().numpy()) and np.array_equal(f, geo.surface_fid.cpu().numpy())
    assert np.array_equal(uv, geo.uv.cpu().numpy()) and np.array_equal(uv_idx, geo.uv_idx.cpu().numpy())
    assert tex.shape == (loop["R"], loop["R"], 3)
    assert float((torch.from_numpy(tex).cuda() - loop["tex"].clamp(0, 1)).abs().max()) <= 0.5 / 255 + 1e-7
    with torch.no_grad():
        textured = _render_textured(loop, torch.from_numpy(tex).cuda(), torch.from_numpy(uv).cuda(), torch.from_numpy(uv_idx).cuda())
    err = (textured - loop["direct"]).abs()[loop["fg"]]
    print(f"exported vs direct: max err {float(err.max()):.5f}, E + 0.5 / 255 = {loop['E'] + 0.5 / 255:.5f}")
    assert float(err.max()) <= loop["E"] + 0.5 / 255


@pytest.mark.gpu
def test_export_needs_materials(loop, tmp_path):
    from tssplat_amd import renderers
    with pytest.raises(AssertionError):
        renderers.MeshRasterizer(loop["geo"]).export(str(tmp_path), "material")


@pytest.mark.gpu
def test_gradient_reaches_only_owned_texels(loop):
    import torch
    from tssplat_amd import dr
    geo = loop["geo"]
    tex = loop["tex"].clone().requires_grad_(True)
    color = _render_textured(loop, tex, geo.uv, geo.uv_idx)
    bg = torch.ones_like(color)
    shaded = dr.antialias(torch.lerp(bg, color, loop["fg"][..., None].float()).contiguous(), loop["rast"], loop["pos_clip"], geo.surface_fid)
    torch.nn.L1Loss()(shaded, torch.zeros_like(shaded)).backward()
    g, owner = tex.grad, loop["owner"]
    assert g is not None and torch.isfinite(g).all()
    assert float(g[owner >= 0].abs().max()) > 0
    assert (g[owner < 0] == 0).all()
