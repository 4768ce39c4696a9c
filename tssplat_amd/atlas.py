"""A textured mesh out of the texture stage: the closed-form per-triangle atlas, the bake of a colour field into it, and
a Wavefront OBJ / MTL / PNG writer and loader.

The reference's ``MeshRasterizer.export`` (renderers/mesh_rasterizer.py:165) takes its UVs from xatlas
(geometry/tetmesh_geometry.py:150-153) and bakes through trimesh and pymeshlab ("trivial per wedge" parameterisation plus a
vertex-colour transfer).  None of the three is used here.  The atlas is pymeshlab's trivial-per-wedge idea in closed form --
one square cell of ``c x c`` texels holds two triangles as mirrored right triangles -- with numbers chosen so that bilinear
sampling never reads a texel of another triangle (include/tssplat_amd.h).  The layout comes from the
library's ``tsamd_atlas_layout`` and the bake is one HIP kernel, one lane per texel; the semantics are restated in float64 in
tests/atlas_oracle.py.  Layout parity with pymeshlab is not a goal.

The PNG is written and read with ``zlib`` and ``struct`` only: 8-bit RGB, ``round(clamp(c, 0, 1) * 255)``, no gamma.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib

import numpy as np
import torch

from . import _capi

__all__ = ["atlas_layout", "atlas_uv", "bake_positions", "bake_material", "write_textured_obj", "load_textured_obj"]

BAKE_CHUNK = 1 << 20          # points per material evaluation of bake_material


def atlas_layout(n_triangles: int, texture_res: int) -> tuple[int, int, int]:
    """``(n, c, L)``: cells per row, texels per cell and texels of leg length for ``n_triangles`` triangles in a square texture
    of ``texture_res`` texels (``tsamd_atlas_layout``).  ``ValueError`` when a cell would have fewer than 6 texels, naming the
    smallest workable resolution ``6 n``."""
    lib = _capi.load()
    n, c, leg = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = lib.tsamd_atlas_layout(int(n_triangles), int(texture_res), C.byref(n), C.byref(c), C.byref(leg))
    if rc != 0:
        if n.value > 0 and c.value < 6:        # (the library fills n, c, L whenever T and R are in range)
            raise ValueError(f"atlas_layout: {int(n_triangles)} triangles do not fit a texture of {int(texture_res)} texels "
                             f"({n.value} cells per row of {c.value} texels, at least 6 are needed): the smallest workable "
                             f"texture_res is {6 * n.value}")
        raise ValueError("atlas_layout: " + lib.tsamd_last_error().decode("utf-8", "replace"))
    return n.value, c.value, leg.value


def atlas_uv(n_triangles: int, texture_res: int, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-wedge UVs of the atlas: ``uv [3 T, 2]`` float32 (``texel / R``, no flip, every corner a texel centre) and
    ``uv_idx [T, 3]`` int32 with ``uv_idx[t] = (3 t, 3 t + 1, 3 t + 2)`` -- usable as ``attr`` and ``tri`` of ``dr.interpolate``
    against a ``rast`` made from the position triangles."""
    T, R = int(n_triangles), int(texture_res)
    n, c, leg = atlas_layout(T, R)
    t = np.arange(T, dtype=np.int64)
    k = t // 2
    origin = np.stack([(k % n) * c, (k // n) * c], -1).astype(np.float64)                       # [T, 2]
    half_a = np.array([[1.5, 1.5], [1.5 + leg, 1.5], [1.5, 1.5 + leg]])
    half_b = np.array([[c - 1.5, c - 1.5], [c - 1.5 - leg, c - 1.5], [c - 1.5, c - 1.5 - leg]])
    corners = np.where((t % 2 == 0)[:, None, None], half_a[None], half_b[None])                 # [T, 3, 2]
    uv = ((origin[:, None, :] + corners) / R).astype(np.float32).reshape(3 * T, 2)
    uv_idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    return torch.from_numpy(uv).to(device), torch.from_numpy(uv_idx).to(device)


def bake_positions(v_pos: torch.Tensor, tri: torch.Tensor, texture_res: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``positions [R, R, 3]`` float32 and ``owner [R, R]`` int32: for every texel of the atlas the surface point it shows
    (barycentrics extrapolated into the gutter) and the triangle that owns it, ``-1`` and position 0 where none does
    (``tsamd_atlas_bake_positions``).  Row ``j``, column ``i`` is texel ``(i, j)``: ``dr.texture``'s orientation."""
    from .tet_spheres_ext import _device_ctx, _stream_ptr
    if not isinstance(v_pos, torch.Tensor) or not v_pos.is_cuda or v_pos.dtype != torch.float32 or v_pos.dim() != 2 or v_pos.shape[1] != 3:
        raise RuntimeError("tssplat_amd.atlas.bake_positions: v_pos must be a float32 [nv, 3] GPU tensor (there is no CPU fallback)")
    if not isinstance(tri, torch.Tensor) or tri.dtype != torch.int32 or tri.dim() != 2 or tri.shape[1] != 3 or tri.device != v_pos.device:
        raise RuntimeError("tssplat_amd.atlas.bake_positions: tri must be an int32 [T, 3] tensor on v_pos's device")
    R, T = int(texture_res), int(tri.shape[0])
    atlas_layout(T, R)                                   # (the ValueError with the smallest workable resolution)
    v_pos, tri = v_pos.detach().contiguous(), tri.contiguous()
    positions = torch.empty((R, R, 3), dtype=torch.float32, device=v_pos.device)
    owner = torch.empty((R, R), dtype=torch.int32, device=v_pos.device)
    with _device_ctx(v_pos.device):
        _capi.check(_capi.load().tsamd_atlas_bake_positions(v_pos.data_ptr(), int(v_pos.shape[0]), tri.data_ptr(), T, R, positions.data_ptr(),
                                                            owner.data_ptr(), _stream_ptr(v_pos.device)))
    return positions, owner


def bake_material(material, v_pos: torch.Tensor, tri: torch.Tensor, texture_res: int) -> torch.Tensor:
    """``tex [R, R, 3]``: ``material(positions=...)["color"]`` at the owned texels of the atlas, evaluated without gradients in
    chunks of at most 2^20 points; unowned texels are 0."""
    with torch.no_grad():
        positions, owner = bake_positions(v_pos, tri, texture_res)
        owned = torch.nonzero(owner.reshape(-1) >= 0)[:, 0]
        points = positions.reshape(-1, 3)
        tex = torch.zeros_like(points)
        for at in range(0, int(owned.shape[0]), BAKE_CHUNK):
            sel = owned[at:at + BAKE_CHUNK]
            tex[sel] = material(positions=points[sel])["color"][..., :3].to(torch.float32)
        return tex.reshape(int(texture_res), int(texture_res), 3)


def _to_numpy(a, dtype):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=dtype)


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def encode_png_rgb8(image: np.ndarray) -> bytes:
    """An ``[H, W, 3]`` uint8 image (row 0 on top) as an 8-bit RGB PNG: filter type 0 on every row, one IDAT chunk."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    h, w = int(image.shape[0]), int(image.shape[1])
    assert image.shape == (h, w, 3)
    rows = np.concatenate([np.zeros((h, 1), np.uint8), image.reshape(h, w * 3)], axis=1)          # (filter byte 0 per row)
    return (_PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def decode_png_rgb8(data: bytes) -> np.ndarray:
    """The inverse of :func:`encode_png_rgb8` for the files it writes (8-bit RGB, not interlaced, filter type 0)."""
    if data[:8] != _PNG_MAGIC:
        raise ValueError("not a PNG file")
    at, header, idat = 8, None, b""
    while at < len(data):
        (size,), tag = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + size]
        if struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] != (zlib.crc32(tag + body) & 0xffffffff):
            raise ValueError("PNG chunk with a wrong CRC")
        if tag == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        at += 12 + size
    if header is None or header[2:] != (8, 2, 0, 0, 0):
        raise ValueError("only the 8-bit RGB, non-interlaced PNG files this module writes are read")
    w, h = header[0], header[1]
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError("only PNG rows of filter type 0 (what this module writes) are read")
    return rows[:, 1:].reshape(h, w, 3).copy()


def texture_to_image(tex) -> np.ndarray:
    """``[R, R, 3]`` float texture (row ``j`` = texel row ``j``) to the uint8 image that is stored: ``round(clamp(c, 0, 1) *
    255)``, no gamma, image rows top-down = texel rows ``R - 1 ... 0`` (viewers put ``v = 0`` at the bottom)."""
    t = _to_numpy(tex, np.float64)
    return np.rint(np.clip(t, 0.0, 1.0) * 255.0).astype(np.uint8)[::-1].copy()


def write_textured_obj(path: str, name: str, v, f, uv, uv_idx, tex) -> None:
    """Writes ``name.obj`` (``v``, ``vt``, ``f a/ta b/tb c/tc`` with 1-based indices, ``mtllib``, ``usemtl``), ``name.mtl``
    (``map_Kd name.png``) and ``name.png`` under ``path``."""
    v, uv = _to_numpy(v, np.float32).reshape(-1, 3), _to_numpy(uv, np.float32).reshape(-1, 2)
    f, uv_idx = _to_numpy(f, np.int64).reshape(-1, 3), _to_numpy(uv_idx, np.int64).reshape(-1, 3)
    if f.shape != uv_idx.shape:
        raise ValueError("write_textured_obj: f and uv_idx must both be [T, 3]")
    os.makedirs(path, exist_ok=True)
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()]              # (9 significant digits: float32 reads back exactly)
    lines += ["vt %.9g %.9g" % tuple(p) for p in uv.tolist()]
    lines += ["f %d/%d %d/%d %d/%d" % (a[0], b[0], a[1], b[1], a[2], b[2]) for a, b in zip((f + 1).tolist(), (uv_idx + 1).tolist())]
    with open(os.path.join(path, name + ".obj"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(os.path.join(path, name + ".mtl"), "w") as fh:
        fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    with open(os.path.join(path, name + ".png"), "wb") as fh:
        fh.write(encode_png_rgb8(texture_to_image(tex)))


def load_textured_obj(path: str, name: str):
    """Reads what :func:`write_textured_obj` wrote: ``(v [nv, 3] f32, f [T, 3] i32, uv [nt, 2] f32, uv_idx [T, 3] i32,
    tex [R, R, 3] f32)`` as numpy arrays, indices 0-based, ``tex`` in ``dr.texture``'s orientation (row ``j`` = texel row ``j``)
    with values ``k / 255``."""
    v, uv, f, uv_idx, png = [], [], [], [], None
    with open(os.path.join(path, name + ".obj")) as fh:
        for line in fh:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w[0] == "vt":
                uv.append([float(x) for x in w[1:3]])
            elif w[0] == "f":
                corners = [c.split("/") for c in w[1:4]]
                f.append([int(c[0]) - 1 for c in corners])
                uv_idx.append([int(c[1]) - 1 for c in corners])
            elif w[0] == "mtllib":
                with open(os.path.join(path, w[1])) as mh:
                    for ml in mh:
                        mw = ml.split()
                        if mw and mw[0] == "map_Kd":
                            png = mw[1]
    if png is None:
        raise ValueError(f"{name}.obj names no material library with a map_Kd texture")
    with open(os.path.join(path, png), "rb") as fh:
        image = decode_png_rgb8(fh.read())
    tex = image[::-1].astype(np.float32) / np.float32(255.0)
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3), np.asarray(uv, np.float32).reshape(-1, 2),
            np.asarray(uv_idx, np.int32).reshape(-1, 3), np.ascontiguousarray(tex))
