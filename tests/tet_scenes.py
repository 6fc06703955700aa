"""Tet scenes for LayeredRenderer.generate's tests: the cases where a tet walk breaks.

``scenes.tet_lattice`` with continuous jitter, seen from outside by the default camera, almost never sends a ray through a
vertex, an edge or a face plane; no tet is missing or flat, no face is duplicated, existence flags are 0 or 1.  Every builder
here post-processes ``tet_lattice``'s output into one of those cases.  Each is a seeded, deterministic function and returns
``(scenes.TetScene, info)``: the scene holds its cameras (``mv``, ``proj``), ``info`` what the tests measure the scene by.

  aligned     no jitter; vertices moved onto pixel rays (fp32), whole z-columns onto one ray; even n, on-axis camera, odd W, H
  holes       a random subset of tets deleted: -1 in face_tets mid-mesh, orphan faces (-1, -1) left in ``faces``
  inside      a camera inside the lattice, and one whose camera plane cuts through faces
  flat        jitter >= 0.5 (inverted, near-flat tets) plus exactly coincident and collinear vertices (zero-area faces)
  duplicates  every k-th face listed twice with the same vertices; the copy is an orphan or takes over the mesh's slot
  deep        small images over deep lattices: tile lists of several LAY_CHUNK, and beyond the plan's TILE_SORT_MAX
  chunk_edge  one tile whose list is k LAY_CHUNK + 1 long and whose last entry is every pixel's first hit (not a lattice)
"""
import dataclasses
import functools
import os
import re

import numpy as np
import torch

from util import ROOT, dm2, scenes

INT_MIN = -2 ** 31
NAMES = ("aligned", "holes", "inside", "flat", "duplicates", "deep")


def thresholds():
    """The list lengths at which the kernels change route, read from the sources: LAY_CHUNK (k_first_intersect's staging
    chunk), TILE_SORT_RANK / TILE_SORT_LDS (the per-tile sorts) and TILE_SORT_MAX (beyond it: one global radix sort)."""
    csrc = os.path.join(ROOT, "dmesh2_renderer_amd", "csrc")
    out = {}
    for name, fn in (("LAY_CHUNK", "dm2_layers.hip"), ("TILE_SORT_RANK", "dm2_binning.hip"), ("TILE_SORT_LDS", "dm2_binning.hip"),
                     ("TILE_SORT_MAX", "dm2_state.h")):
        src = open(os.path.join(csrc, fn)).read()
        out[name] = int(re.search(r"constexpr \w+ %s = (\d+);" % name, src).group(1))
    return out


def renderer(ts, device="cpu", **kw):
    """The scene's LayeredRenderer (ray tensors on ``device``)."""
    kw.setdefault("fused_prep", False)
    return dm2.LayeredRenderer(ts.mv.to(device), ts.proj.to(device), ts.width, ts.height, device, **kw)


def _replace(ts, **kw):
    kw = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return dataclasses.replace(ts, **kw)


def hull_faces(ts):
    """(F,) bool: faces with exactly one tet (the mesh's outer surface, for an untouched lattice)."""
    ft = ts.face_tets.numpy()
    return (ft >= 0).sum(1) == 1


# ---- existence tables ----------------------------------------------------------------------------------------------------
ODD_VALUES = (0, 1, 2, -1, INT_MIN)


def existence_tables(F, seed):
    """name -> (F,) int32: all 0, all 1, and a seeded mix of 0, 1 and values other than 0 / 1 (2, -1, INT_MIN: any non-zero
    value means "exists")."""
    rng = np.random.RandomState(seed)
    return dict(zeros=np.zeros(F, np.int32), ones=np.ones(F, np.int32),
                odd=np.asarray(ODD_VALUES, np.int64)[rng.randint(0, len(ODD_VALUES), F)].astype(np.int32))


def with_existence(ts, table):
    return _replace(ts, faces_existence=np.asarray(table, np.int32))


# ---- aligned ---------------------------------------------------------------------------------------------------------------
def aligned(W=65, H=49, n=4, seed=1, share=0.7, tol=0.45):
    """An unjittered lattice whose vertices sit on camera 0's pixel rays: ray_o + t ray_d of the pixel the vertex projects
    into, in fp32, from the LayeredRenderer's own ray tensors.  A seeded ``share`` of the z-columns is moved as a whole onto
    the ray of the column's middle vertex (the ray then runs along the column's edges), the vertices of the other columns
    each onto their own pixel's ray; a vertex that would move by more than ``tol`` cells stays.  n even, the camera on the
    axis, W and H odd: the central column's and row's rays lie in the lattice planes x = 0 and y = 0."""
    assert n % 2 == 0 and W % 2 == 1 and H % 2 == 1
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + 9000 + seed, jitter=0.0, existence_p=0.5, num_cams=2)
    lr = renderer(ts)
    ro, rd = lr.ray_o[0].numpy(), lr.ray_d[0].numpy()
    _, img = lr.compute_verts_ndc_image(ts.verts, ts.mv[:1], ts.proj[:1])
    img = img[0].numpy()
    px = np.clip(np.floor(img[:, 0]), 0, W - 1).astype(np.int64)
    py = np.clip(np.floor(img[:, 1]), 0, H - 1).astype(np.int64)
    v = ts.verts.numpy().copy()
    m, cell = n + 1, 2.0 / n
    rng = np.random.RandomState(seed)
    pixel_of = np.full((len(v), 2), -1, np.int64)
    columns = 0
    for col in range(m * m):
        ids = col * m + np.arange(m)
        whole = rng.uniform() < share
        moved = 0
        for vid in ids:
            c = ids[m // 2] if whole else vid
            o, d = ro[py[c], px[c]].astype(np.float64), rd[py[c], px[c]].astype(np.float64)
            t = np.dot(v[vid].astype(np.float64) - o, d)
            p = (o + t * d).astype(np.float32)
            if np.abs(p.astype(np.float64) - v[vid]).max() <= tol * cell:
                v[vid] = p
                pixel_of[vid] = (px[c], py[c])
                moved += 1
        columns += int(whole and moved == m)
    return _replace(ts, verts=v), dict(pixel_of=pixel_of, columns=columns, on_ray=int((pixel_of[:, 0] >= 0).sum()))


# ---- holes -----------------------------------------------------------------------------------------------------------------
def delete_tets(ts, kill):
    """``ts`` without the tets of the (T,) bool mask: tets and tet_faces lose their rows, face_tets is renumbered and gets -1
    where a tet went (in the slot it had: (-1, t) occurs as well as (t, -1)); faces is untouched, so a face that lost every
    tet stays as an orphan (-1, -1)."""
    kill = np.asarray(kill, bool)
    new_id = np.where(kill, -1, np.cumsum(~kill) - 1).astype(np.int32)
    ft = ts.face_tets.numpy().copy()
    ft[ft >= 0] = new_id[ft[ft >= 0]]
    return _replace(ts, tets=ts.tets.numpy()[~kill], tet_faces=ts.tet_faces.numpy()[~kill], face_tets=ft)


def holes(W=90, H=70, n=5, seed=2, density=0.25, jitter=0.2, existence_p=0.6):
    """A lattice with a seeded random ``density`` of its tets deleted.  Camera 0 is the default one: every first hit is a
    face of the lattice's hull, an orphan where its tet went.  Camera 1 sits inside the lattice near its front: the plan
    culls what lies between it and its near plane, so its first hits are interior faces -- with two tets, with one (met from
    the side of the tet or from the side without), and orphans."""
    full = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + 9100 + seed, jitter=jitter, existence_p=existence_p, num_cams=1)
    rng = np.random.RandomState(1000 + seed)
    kill = rng.uniform(size=full.tets.shape[0]) < density
    ts = delete_tets(full, kill)
    ts = _replace(ts, mv=torch.stack([full.mv[0], _look((0.07, -0.04, 0.93))]), proj=full.proj[:1].repeat(2, 1, 1))
    ft = ts.face_tets.numpy()
    return ts, dict(hull=hull_faces(full), orphan=(ft < 0).all(1), one_tet=(ft >= 0).sum(1) == 1, killed=int(kill.sum()))


# ---- inside ----------------------------------------------------------------------------------------------------------------
def _look(position, yaw=0.0, pitch=0.0):
    """A model-view matrix of a camera at ``position`` that looks down -z turned by ``yaw`` about y, then ``pitch`` about x
    (radians): mv = R^T translate(-position)."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    r = ry @ rx                                                       # camera axes in world coordinates (columns)
    mv = np.eye(4)
    mv[:3, :3] = r.T
    mv[:3, 3] = -r.T @ np.asarray(position, np.float64)
    return torch.from_numpy(mv.astype(np.float32))


def inside(W=75, H=53, n=5, seed=3, jitter=0.2, existence_p=0.5):
    """Camera 0 sits inside the lattice, turned off the axes; camera 1 sits in it too, unturned, so that its camera plane
    z = const cuts a layer of cells: the faces of that layer straddle the plane (some vertices project mirrored, with
    NDC z > 1)."""
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + 9200 + seed, jitter=jitter, existence_p=existence_p, num_cams=1)
    mvs = torch.stack([_look((0.13, -0.21, 0.37), yaw=0.45, pitch=-0.2), _look((0.05, 0.1, 0.02))])
    return _replace(ts, mv=mvs, proj=ts.proj[:1].repeat(2, 1, 1)), dict(plane_cam=1)


def straddlers(ts, cam):
    """(F,) bool: faces with vertices on both sides of camera ``cam``'s plane (view z = 0)."""
    v = np.concatenate([ts.verts.numpy().astype(np.float64), np.ones((len(ts.verts), 1))], 1)
    z = (v @ ts.mv[cam].numpy().astype(np.float64).T)[:, 2]
    zf = z[ts.faces.numpy()]
    return (zf.max(1) > 0) & (zf.min(1) < 0)


# ---- flat ------------------------------------------------------------------------------------------------------------------
def flat(W=90, H=70, n=5, seed=4, jitter=0.6, existence_p=0.6, handful=6):
    """Jitter beyond half a cell (inverted and near-zero-volume tets) plus ``handful`` vertex pairs made exactly coincident and
    ``handful`` triples made exactly collinear (coordinates on the 2^-7 grid, the middle one their exact midpoint): zero-area
    faces, whose normal is the zero vector after the walk's fmaxf(n_norm, 1e-4) clamp."""
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + 9300 + seed, jitter=jitter, existence_p=existence_p, num_cams=2)
    v = ts.verts.numpy().copy()
    faces = ts.faces.numpy()
    rng = np.random.RandomState(2000 + seed)
    used = set()
    done_pairs = done_triples = 0
    while done_pairs < handful or done_triples < handful:
        a, c, b = (int(x) for x in faces[rng.randint(0, len(faces))])
        if used & {a, b, c}:
            continue
        used |= {a, b, c}
        if done_pairs < handful:
            v[c] = v[a]                                                # coincident: the edge a-c has length 0
            done_pairs += 1
        else:
            v[a] = np.round(v[a] * 64) / 64
            v[b] = np.round(v[b] * 64) / 64
            v[c] = (v[a] + v[b]) * np.float32(0.5)                     # exact on the 2^-7 grid: a, c, b collinear
            done_triples += 1
    return _replace(ts, verts=v), dict(touched=sorted(used))


def face_normal_norms(ts):
    """(F,) float32 |cross(p1 - p0, p2 - p0)| as tet_face_outward_normal computes it."""
    v, f = ts.verts.numpy(), ts.faces.numpy()
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def tet_volumes(ts):
    """(T,) float64 signed volumes (an untouched Kuhn lattice has one sign per axis permutation; jitter flips some)."""
    v, t = ts.verts.numpy().astype(np.float64), ts.tets.numpy()
    a, b, c = (v[t[:, i]] - v[t[:, 0]] for i in (1, 2, 3))
    return np.einsum("ij,ij->i", np.cross(a, b), c) / 6.0


# ---- duplicates ------------------------------------------------------------------------------------------------------------
def duplicates(W=90, H=70, n=5, seed=5, k=4, jitter=0.2, existence_p=0.6):
    """Every k-th face appended again under a new id with the same vertices.  Copies cycle through three kinds: an orphan
    (face_tets (-1, -1), in no tet's tet_faces); the mesh's real face (it takes over the original's face_tets row and its
    places in tet_faces; the original becomes the orphan); and a miswired one (the tets list the copy in tet_faces, but
    face_tets still gives the tets to the original: a walk that stands on the original does not find it among its tet's four
    faces, cnt != 3).  A face and its copy have equal min-depth keys and equal t: the order of the tile list (emission
    order: the lower id first) alone decides which one is the first hit."""
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + 9400 + seed, jitter=jitter, existence_p=existence_p, num_cams=2)
    faces, ft, tf = ts.faces.numpy(), ts.face_tets.numpy().copy(), ts.tet_faces.numpy().copy()
    F = faces.shape[0]
    src = np.arange(0, F, k)
    copy = F + np.arange(len(src))
    kind = np.arange(len(src)) % 3                                     # 0 orphan copy, 1 the copy is the mesh's face, 2 miswired
    real, miswired = kind == 1, kind == 2
    ft2 = np.concatenate([ft, np.full((len(src), 2), -1, ft.dtype)])
    ft2[copy[real]] = ft[src[real]]
    ft2[src[real]] = -1
    remap = np.arange(F)
    remap[src[real]] = copy[real]
    remap[src[miswired]] = copy[miswired]
    rng = np.random.RandomState(3000 + seed)
    ex = np.concatenate([ts.faces_existence.numpy(), (rng.uniform(size=len(src)) < existence_p).astype(np.int32)])
    dup = np.zeros(F + len(src), bool)
    dup[src] = dup[copy] = True
    out = _replace(ts, faces=np.concatenate([faces, faces[src]]), face_tets=ft2, tet_faces=remap[tf].astype(np.int32), faces_existence=ex)
    return out, dict(dup=dup, src=src, copy=copy, real=real, miswired=miswired)


# ---- deep ------------------------------------------------------------------------------------------------------------------
def deep(W=32, H=32, n=14, seed=6, jitter=0.2, existence_p=0.3, num_cams=1):
    """A small image over a deep lattice: every tile's face list is many LAY_CHUNKs long.  n = 14 at 32 x 32 gives lists of
    several thousand entries; n = 25 puts the longest one beyond TILE_SORT_MAX (the plan's global-sort route)."""
    ts = scenes.tet_lattice(W, H, n, seed=scenes.SEED_BASE + 9500 + seed, jitter=jitter, existence_p=existence_p, num_cams=num_cams)
    return ts, {}


def chunk_edge(k=1, seed=7):
    """One 16 x 16 tile whose face list has exactly k LAY_CHUNK + 1 entries, the last of which is every pixel's first hit: a
    fronto-parallel back triangle over the whole tile (the one tet's front face, with the highest face id: its min-depth key
    ties with the tet's side faces, so it is listed last) behind k LAY_CHUNK - 3 orphan slivers at pixel corners, nearer and
    covering no pixel centre.  The first-hit loop's last chunk holds that single entry."""
    W = H = 16
    chunk = thresholds()["LAY_CHUNK"]
    n_small = k * chunk - 3
    rng = np.random.RandomState(seed)
    t = scenes.TAN_HALF_FOV

    def world(px, py, depth):                                           # image point at view depth -> world (camera at z = CAM_DIST)
        return [(px / W * 2.0 - 1.0) * depth * (W / H) * t, (py / H * 2.0 - 1.0) * depth * t, scenes.CAM_DIST - depth]

    verts, faces = [], []
    for i in range(n_small):
        cx, cy = rng.randint(1, W), rng.randint(1, H)                   # a pixel corner
        depth = 2.0 + 0.5 * (i + 1) / (n_small + 1)
        b = len(verts)
        verts += [world(cx - 0.2, cy - 0.1, depth), world(cx + 0.2, cy - 0.1, depth + 0.001), world(cx, cy + 0.2, depth + 0.002)]
        faces.append([b, b + 1, b + 2])
    b = len(verts)
    verts += [world(-20.0, -20.0, 3.0), world(60.0, -20.0, 3.0), world(-20.0, 60.0, 3.0), world(8.0, 8.0, 4.0)]
    sides = [[b, b + 1, b + 3], [b + 1, b + 2, b + 3], [b, b + 2, b + 3]]
    faces += sides + [[b, b + 1, b + 2]]
    F = len(faces)
    face_tets = np.full((F, 2), -1, np.int32)
    face_tets[F - 4:, 0] = 0
    mv, proj = scenes.camera(W, H)
    ts = scenes.TetScene(W, H, mv[None], proj[None], torch.tensor(verts, dtype=torch.float32), torch.tensor(faces, dtype=torch.int32),
                         torch.tensor([[b, b + 1, b + 2, b + 3]], dtype=torch.int32), torch.from_numpy(face_tets),
                         torch.tensor([[F - 1, F - 4, F - 3, F - 2]], dtype=torch.int32), torch.ones(F, dtype=torch.int32))
    return ts, dict(back=F - 1, entries=k * chunk + 1)


def build(name, **kw):
    return globals()[name](**kw)


# the cases the tests run: name -> (builder, arguments)
CASES = dict(aligned=("aligned", {}), holes=("holes", {}), inside=("inside", {}), flat=("flat", {}), duplicates=("duplicates", {}),
             deep=("deep", {}), deep_sort=("deep", dict(n=25)), chunk_edge=("chunk_edge", {}), chunk_edge3=("chunk_edge", dict(k=3)))
FIXED_SIZE = ("deep_sort", "chunk_edge", "chunk_edge3")                 # cases built for one image size


@functools.lru_cache(maxsize=None)
def case(name, W=None, H=None):
    """Case ``name`` (at another image size when given) -> (TetScene, info).  Cached: treat the tensors as read-only."""
    builder, kw = CASES[name]
    if W is not None:
        kw = dict(kw, W=W, H=H)
    return build(builder, **kw)
