"""Seeded general cameras and scenes re-posed under them, for the tests (a helper module, numpy and torch only).

Every camera of ``scenes.camera`` is an identity rotation plus a translation with the five-entry symmetric OpenGL
perspective: under it most of the 4x4 arithmetic of the fused prep and of the analytic rays multiplies by exact zeros or by
a symmetric block, so that a wrong index, a transposed rotation or a reassociated sum changes no bit.  The cameras here
have a three-axis rotation (``pose``: no zero in mv[:3, :4], a clearly asymmetric rotation block) and an off-axis,
non-square, sheared pinhole (``pinhole``); the scenes are ``scenes.triangle_soup`` / ``scenes.tet_lattice`` moved into
world space so that such a camera sees them as they were built.

  pose, pinhole      the matrices
  soup_cameras       ``cams`` general cameras: camera 0 and seeded perturbations of its pose and intrinsics
  reposed_soup       triangle_soup as general camera 0 sees it; both windings; faces_intense per view      (rendered)
  grazing_soup       the same plus one camera turned until its w = 0 plane cuts the soup; dense mix        (prep only)
  reposed_lattice    tet_lattice as general camera 0 sees it                                               (rendered)
"""
import dataclasses
import math

import numpy as np
import torch

from util import scenes

NEAR = 1.0      # the rays take no perspective divide: they are pixel rays only with the near plane at 1 (scenes.Z_NEAR)
FAR = 10.0
W_EPS = 1e-4    # the projection's |w| clamp

# pose 0: all three angles well away from 0 and pi/2
POSE0 = dict(rx=0.35, ry=-0.5, rz=0.6, t=(0.4, -0.3, -0.25))
# near-identity sensor mixes (left factors of proj).  Rows 0-1: in-plane roll / shear, a little of clip z and w in x and y;
# last row (0, 0, 0, 1): w is untouched.  RENDERED keeps row 2 = (0, 0, 1, 0) (the un-projected near point keeps w = 1);
# DENSE mixes x, y and w into clip z as well (prep only).
MIX_RENDERED = ((1.0, 0.03, 0.004, -0.02), (-0.025, 1.0, -0.003, 0.015), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
MIX_DENSE = ((1.0, 0.03, 0.004, -0.02), (-0.025, 1.0, -0.003, 0.015), (0.02, -0.015, 1.0, 0.01), (0.0, 0.0, 0.0, 1.0))


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    m = np.eye(4)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def pose64(rx, ry, rz, t):
    m = np.eye(4)
    m[:3, 3] = np.asarray(t, np.float64)
    return m @ _rot("z", rz) @ _rot("y", ry) @ _rot("x", rx)


def pose(rx, ry, rz, t):
    """mv (4,4) float32 = translate(t) @ Rz @ Ry @ Rx (column-vector convention, as scenes.camera)."""
    return torch.from_numpy(pose64(rx, ry, rz, t).astype(np.float32))


def pinhole64(W, H, fx, fy, cx, cy, far, mix=None):
    n, f = NEAR, float(far)
    p = np.zeros((4, 4))
    p[0, 0], p[1, 1] = 2.0 * fx / W, 2.0 * fy / H
    p[0, 2], p[1, 2] = cx, cy
    p[2, 2], p[2, 3] = -(f + n) / (f - n), -2.0 * f * n / (f - n)
    p[3, 2] = -1.0
    if mix is not None:
        mix = np.asarray(mix, np.float64)
        assert mix.shape == (4, 4) and np.array_equal(mix[3], [0.0, 0.0, 0.0, 1.0])
        p = mix @ p
    return p


def pinhole(W, H, fx, fy, cx, cy, far, mix=None):
    """proj (4,4) float32: OpenGL clip-space pinhole, focal lengths fx, fy in pixels (proj[0,0] = 2 fx / W, proj[1,1] =
    2 fy / H; scenes.camera is fx = fy = H), principal-point offset proj[0,2] = cx, proj[1,2] = cy in NDC units, near plane
    at 1, left-multiplied by ``mix`` (4,4, last row (0,0,0,1))."""
    return torch.from_numpy(pinhole64(W, H, fx, fy, cx, cy, far, mix).astype(np.float32))


def soup_cameras(W, H, seed, cams, mix=MIX_RENDERED, spread=1.0):
    """-> mv, proj (cams,4,4) float32.  Camera 0: POSE0 and a pinhole close to scenes.camera's (fx = 1.04 H, fy = 0.97 H,
    off-axis).  Cameras 1..: pose 0 with every angle and offset perturbed (seeded, ``spread`` x 0.03 rad / 0.05 units), each
    with its own fx / fy and principal point, so that pixels are not square and no two views share a proj."""
    rng = np.random.RandomState(seed)
    mvs, projs = [], []
    for c in range(cams):
        k = 0.0 if c == 0 else spread
        ang = [POSE0[a] + k * rng.uniform(-0.03, 0.03) for a in ("rx", "ry", "rz")]
        t = np.asarray(POSE0["t"]) + k * rng.uniform(-0.05, 0.05, 3)
        fx = H * (1.04 + k * rng.uniform(-0.04, 0.04))
        fy = H * (0.97 + k * rng.uniform(-0.04, 0.04))
        cx, cy = 0.04 + k * rng.uniform(-0.03, 0.03), -0.03 + k * rng.uniform(-0.03, 0.03)
        mvs.append(pose(*ang, t))
        projs.append(pinhole(W, H, fx, fy, cx, cy, FAR, mix))
    return torch.stack(mvs), torch.stack(projs)


def _to_world(verts, mv_built, mv0):
    """World positions that ``mv0`` takes to the view-space positions ``mv_built`` gives ``verts`` (float64 throughout)."""
    v = np.asarray(verts, np.float64)
    hom = np.concatenate((v, np.ones((v.shape[0], 1))), axis=1)
    view = hom @ np.asarray(mv_built, np.float64).T
    world = view @ np.linalg.inv(np.asarray(mv0, np.float64)).T
    return world[:, :3]


def reposed_soup(W, H, F, seed, cams, mix=MIX_RENDERED, **soup_kw):
    """scenes.triangle_soup(W, H, F, seed, **soup_kw) as general camera 0 of ``soup_cameras`` sees it -> SoupScene with
    ``cams`` cameras, every other face reversed (both windings after projection), faces_intense drawn per view."""
    sc = scenes.triangle_soup(W, H, F, seed, num_cams=1, **soup_kw)
    mv, proj = soup_cameras(W, H, seed + 1, cams, mix)
    world = _to_world(sc.verts.numpy(), sc.mv[0].numpy(), mv[0].numpy())
    faces = sc.faces.clone()
    faces[1::2] = faces[1::2][:, [0, 2, 1]]
    g = torch.Generator().manual_seed(seed + 2)
    intense = torch.rand((cams, F), generator=g, dtype=torch.float32) * 0.5 + 0.75
    return dataclasses.replace(sc, mv=mv, proj=proj, verts=torch.from_numpy(world.astype(np.float32)), faces=faces,
                               faces_intense=intense)


GRAZE_TURN = 1.15       # rad about the camera's own y axis: the soup spans +-0.67 rad of view 0
GRAZE_CLAMPED = 32      # vertices placed inside the |w| clamp
GRAZE_BAND = 0.05       # no other vertex has |w| below this


def grazing_soup(W, H, F, seed, cams, mix=MIX_DENSE, **soup_kw):
    """reposed_soup plus one last camera: camera 0 turned by GRAZE_TURN about its own y axis, so that its w = 0 plane cuts
    the soup (part of it has w < 0).  The GRAZE_CLAMPED vertices nearest that plane are moved along its normal to
    1e-5 <= |w| <= 8e-5, alternating in sign (both clamp branches, far from either threshold in fp32), every other vertex
    with |w| < GRAZE_BAND out to the band's edge.  The band keeps float64 a reference for the fp32 gradients at 1e-5 of the
    largest entry: the fp32 w is off by about 8 u A_w = 2.4e-6 (A_w = 5, the sum of |products| in w), the gradient through w
    goes with 1 / w^2, so an unclamped vertex carries an error of 2 (2.4e-6 / |w|) / w^2 against the 1 / 1e-4 of a clamped
    vertex's entries: 4e-6 of them at |w| = 0.05 (6e-5 at 0.02, and some thirty vertices sit on the band's edge).  Prep only
    (the view is not renderable)."""
    sc = reposed_soup(W, H, F, seed, cams, mix, **soup_kw)
    mv0 = sc.mv[0].numpy().astype(np.float64)
    mvg = _rot("y", GRAZE_TURN) @ mv0
    prg = pinhole64(W, H, 0.93 * H, 1.06 * H, -0.05, 0.035, FAR, mix)
    row = (prg @ mvg)[3]                                             # w = row . (x, y, z, 1)
    v = sc.verts.numpy().astype(np.float64)
    w = v @ row[:3] + row[3]
    step = row[:3] / (row[:3] @ row[:3])                             # moves w by one unit
    near = np.argsort(np.abs(w), kind="stable")
    rng = np.random.RandomState(seed + 3)
    target = rng.uniform(1e-5, 8e-5, GRAZE_CLAMPED) * np.where(np.arange(GRAZE_CLAMPED) % 2 == 0, 1.0, -1.0)
    clamped = near[:GRAZE_CLAMPED]
    v[clamped] += (target - w[clamped])[:, None] * step
    rest = near[GRAZE_CLAMPED:]
    inside = rest[np.abs(w[rest]) < GRAZE_BAND]
    v[inside] += (np.where(w[inside] >= 0, GRAZE_BAND, -GRAZE_BAND) * 1.01 - w[inside])[:, None] * step
    g = torch.Generator().manual_seed(seed + 4)
    intense = torch.cat((sc.faces_intense, torch.rand((1, F), generator=g, dtype=torch.float32) * 0.5 + 0.75))
    return dataclasses.replace(sc, mv=torch.cat((sc.mv, torch.from_numpy(mvg.astype(np.float32))[None])),
                               proj=torch.cat((sc.proj, torch.from_numpy(prg.astype(np.float32))[None])),
                               verts=torch.from_numpy(v.astype(np.float32)), faces_intense=intense)


def reposed_lattice(W, H, n, seed, cams, **lattice_kw):
    """scenes.tet_lattice(W, H, n, seed, **lattice_kw) as general camera 0 of ``soup_cameras`` sees it -> TetScene."""
    ts = scenes.tet_lattice(W, H, n, seed, num_cams=1, **lattice_kw)
    mv, proj = soup_cameras(W, H, seed + 1, cams, MIX_RENDERED)
    world = _to_world(ts.verts.numpy(), ts.mv[0].numpy(), mv[0].numpy())
    return dataclasses.replace(ts, mv=mv, proj=proj, verts=torch.from_numpy(world.astype(np.float32)))
