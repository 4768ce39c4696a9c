"""Numpy / plain-Python statement of the merge's flood fill (tssplat_amd/merge.py: ``components``, ``fill_field``, ``merge_tets(fill=)``;
include/tssplat_amd.h, "Flood fill").  Everything is integers and bits: the device results equal this file's bit for bit.

Connectivity is the extraction's own (tests/union_oracle.py): two nodes are adjacent iff they differ by ``+-(di, dj, dk)`` with
``(di, dj, dk)`` in ``{0, 1}^3`` without 0 -- the seven owned Kuhn edges of a node and their reverses, 14 neighbours; ``(1, -1, 0)``
and its kin are NOT edges.  A node is inside iff ``field > level`` (a NaN is outside).  A component is a maximal set of nodes with
equal inside bit connected through these edges.  Under this connectivity, and no other, node components and surface components
correspond: a closed extraction has (#inside components + #outside components - 1) connected surfaces.

The labelling is a sequential union-find over the owned edges, not a repeated whole-grid sweep.  (A pitfall of the sweep, met
when this was written: with ``a = lab[:-1]`` and ``b = lab[1:]`` two views of one array, assigning ``where(same, minimum(a, b), .)``
to both ends in place reaches a false fixed point, because the views overlap and the second write can raise a value the first
one just lowered.  A sweep has to take ``minimum`` with the CURRENT value at each write.)
"""
import numpy as np

import union_oracle as U

MODES = ("cavities", "outer")
OWNED = tuple(((m >> 2) & 1, (m >> 1) & 1, m & 1) for m in range(1, 8))


def _edges(inside):
    """int64 ``[E, 2]``: the flat indices of the ends of every owned edge whose ends have equal inside bit."""
    G = inside.shape[0]
    idx = np.arange(G ** 3, dtype=np.int64).reshape(G, G, G)
    out = []
    for di, dj, dk in OWNED:
        a = (slice(0, G - di), slice(0, G - dj), slice(0, G - dk))
        b = (slice(di, G), slice(dj, G), slice(dk, G))
        same = inside[a] == inside[b]
        out.append(np.stack([idx[a][same], idx[b][same]], 1))
    return np.concatenate(out)


def _label_mask(inside):
    """int32 ``[G, G, G]``: the smallest flat index of each node's component of the boolean grid ``inside``."""
    G = inside.shape[0]
    parent = list(range(G ** 3))
    for a, b in _edges(inside).tolist():
        while parent[a] != a:                      # find with path halving
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:                                  # the smaller root stays a root: a root is its tree's minimum
            parent[b] = a
        elif b < a:
            parent[a] = b
    for n in range(G ** 3):                        # a parent is smaller than its child, so it is final already
        parent[n] = parent[parent[n]]
    return np.asarray(parent, dtype=np.int32).reshape(G, G, G)


def components(field, level):
    """int32 ``[G, G, G]``: ``label[n]`` = the smallest flat index ``(i G + j) G + k`` in the component of ``n``; inside and outside nodes
    in one pass."""
    return _label_mask(U.occupancy(field, level))


def _border(G):
    b = np.ones((G, G, G), dtype=bool)
    b[1:-1, 1:-1, 1:-1] = False
    return b


def fill_field(field, level, mode):
    """``dict(field, cavities, cavity_nodes, islands, island_nodes)``.  The exterior is every outside component with a node on the
    grid's border.  ``"cavities"``: solid = every node that is not exterior.  ``"outer"``: of that solid, only the component with the
    most nodes (ties: the smaller label).  New field: unchanged inside bit, unchanged bits; outside -> inside ``+inf``; inside ->
    outside ``-inf``."""
    assert mode in MODES
    f = np.ascontiguousarray(np.asarray(field, dtype=np.float32))
    G = f.shape[0]
    inside = U.occupancy(f, level)
    label = _label_mask(inside)
    exterior_labels = np.unique(label[~inside & _border(G)])
    exterior = ~inside & np.isin(label, exterior_labels)
    solid = ~exterior
    cavity = solid & ~inside
    cavities, cavity_nodes = int(np.unique(label[cavity]).size), int(cavity.sum())
    islands = island_nodes = 0
    if mode == "outer" and solid.any():
        label2 = _label_mask(solid)
        labs, counts = np.unique(label2[solid], return_counts=True)        # ascending labels: argmax takes the smaller on ties
        keep = solid & (label2 == labs[int(np.argmax(counts))])
        islands, island_nodes = int(labs.size - 1), int(solid.sum() - keep.sum())
        solid = keep
    out = f.copy()
    out[solid & ~inside] = np.inf
    out[~solid & inside] = -np.inf
    return {"field": out, "cavities": cavities, "cavity_nodes": cavity_nodes, "islands": islands, "island_nodes": island_nodes}


def mesh_components(n_vertices, faces):
    """int64 ``[Nv]``: per vertex the smallest vertex index of its connected surface component (vertices joined by triangles)."""
    parent = list(range(int(n_vertices)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for x, y in ((a, b), (b, c)):
            x, y = find(x), find(y)
            if x < y:
                parent[y] = x
            elif y < x:
                parent[x] = y
    return np.asarray([find(x) for x in range(int(n_vertices))], dtype=np.int64)


def count_mesh_components(n_vertices, faces):
    return int(np.unique(mesh_components(n_vertices, faces)).size)


def submesh_of(v_sub, f_sub, v_all, f_all):
    """True iff (v_sub, f_sub) is (v_all, f_all) without some whole connected components: the kept vertices with the same bits in the
    same order, the kept triangles in the same order after renumbering."""
    v_sub, v_all = np.asarray(v_sub, dtype=np.float32), np.asarray(v_all, dtype=np.float32)
    f_sub, f_all = np.asarray(f_sub, dtype=np.int64).reshape(-1, 3), np.asarray(f_all, dtype=np.int64).reshape(-1, 3)
    comp = mesh_components(len(v_all), f_all)
    # greedy match in order: vertex bits are positions on distinct grid edges, so equal rows of one mesh do not occur off-node
    keep_v = np.zeros(len(v_all), dtype=bool)
    rows_all = v_all.view(np.uint32).reshape(-1, 3)
    rows_sub = v_sub.view(np.uint32).reshape(-1, 3)
    at = 0
    for row in rows_sub:
        while at < len(rows_all) and not np.array_equal(rows_all[at], row):
            at += 1
        if at == len(rows_all):
            return False
        keep_v[at] = True
        at += 1
    kept_comps = np.unique(comp[keep_v])
    if not np.array_equal(keep_v, np.isin(comp, kept_comps)):               # whole components only
        return False
    new_id = np.cumsum(keep_v) - 1
    keep_f = keep_v[f_all[:, 0]] if len(f_all) else np.zeros(0, dtype=bool)
    return np.array_equal(new_id[f_all[keep_f]].reshape(-1, 3), f_sub)


def merge_tets(tet_v, elem, grid=128, bounds=None, level=None, fill="none"):
    """``U.merge_tets`` with the fill between the field and the extraction: its dict, of the field that was extracted, plus ``fill`` and
    the four counts."""
    m = U.merge_tets(tet_v, elem, grid, bounds, level)
    m.update(fill=fill, cavities=0, cavity_nodes=0, islands=0, island_nodes=0)
    if fill == "none":
        return m
    filled = fill_field(m["field"], m["level"], fill)
    field = filled.pop("field")
    v, faces, closed = U.extract_surface(field, m["bounds"], m["level"])
    m.update(filled, field=field, v=v, faces=faces, closed=closed, inside_fraction=int(U.occupancy(field, m["level"]).sum()) / float(grid ** 3))
    return m
