"""Far off-screen geometry: triangles with corners 1e2 to 1e7 px away from the pixels they are tested on.

The reference culls a face only when all three of its NDC z lie outside [-1, 1] (forward.cu:71).  Faces that cross the side of
the frustum near the camera, faces with a vertex whose |w| the projection clamps to 1e-4 and faces with a vertex behind the
camera are therefore binned, composited and differentiated with image coordinates far outside the frame: a camera inside or
close to the mesh, the normal case of an optimised scene.  There the rounding of the clippers' corner coordinates (p0 + t e), of
the crossing parameters ((w - p0) r) and of the normal_c table grows with the triangle's coordinates, not with the pixel's.

Seeded, numpy-only generators; tests/test_far_geometry.py checks on the CPU what they claim:
  far_triangle / far_pairs   (triangle, pixel) pairs for the device clippers (tests/test_gpu_clippers.py, tests/structured.py)
  inside_scene               a lattice of faces around a camera inside it (tests/test_gpu_offscreen.py)
"""
import numpy as np

REACHES = (1e2, 1e4, 1e6, 1e7)
BASES = (0.0, 1900.0, 3800.0)          # tested pixels near the origin, at 1080p and at 4K magnitudes
KINDS = ("wedge", "sliver", "corner", "line", "axis")
STRESS = ("corner", "line", "axis")
# components of the short side of an "axis" edge: exactly 0, inside the 1e-3 "iszero" threshold, just above it, below 1/64
# (FAST_TIE_NEAR of dm2_clip_fast.h) and well above it
AXIS_OFFSETS = (0.0, 2.5e-4, 9e-4, 1.01e-3, 1.5e-2, 0.2, 2.0)


def jit(x, k):
    """fp32 ``x`` moved by ``k`` ulp."""
    x = np.float32(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.float32(np.inf) if k > 0 else np.float32(-np.inf))
    return x


def _dir(th):
    return np.array([np.cos(th), np.sin(th)])


def far_triangle(rng, pm, reach, kind):
    """One triangle (fp32 (3, 2), in no particular winding) of construction ``kind`` around the pixel whose min corner is
    ``pm`` (integers):
      wedge   one corner in or next to the pixel, two at ~reach in random directions (the pixel near the apex);
      sliver  two corners in or next to the pixel, one at ~reach;
      corner  a long edge EXACTLY through a corner of the pixel (all three points of it on the quarter-pixel or integer
              lattice, collinear in exact arithmetic), half of them with the far end moved by 1-3 ulp;
      line    the near corner exactly on one of the pixel's lines, or 1 ulp off it, the others at ~reach or near;
      axis    a long edge nearly parallel to an axis: its short component one of AXIS_OFFSETS over ~reach."""
    pm = np.asarray(pm, np.float64)
    far = lambda: reach * rng.uniform(0.7, 1.0)
    near = pm + rng.uniform(-0.5, 1.5, 2)
    th = rng.uniform(0, 2 * np.pi)
    spread = rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 2.5)
    if kind == "wedge":
        tri = [near, near + far() * _dir(th), near + far() * _dir(th + spread)]
    elif kind == "sliver":
        tri = [near, near + rng.uniform(-3, 3, 2), near + far() * _dir(th)]
    elif kind == "corner":
        cc = rng.randint(0, 2, 2)
        c = pm + cc
        # a direction into the pixel from that corner (or out of it), now and then along one of its lines
        d = rng.randint(1, 5, 2) * (1 - 2 * cc) * rng.choice([-1, 1]) * (rng.rand(2) > [0.1, 0.1]).astype(np.float64)
        if not d.any():
            d[rng.randint(0, 2)] = 1.0 - 2 * cc[0]
        a = c - d * rng.choice([0.25, 0.5, 1.0])
        f = c + d * np.floor(far() / np.hypot(*d))
        if rng.randint(0, 2):
            j = rng.randint(0, 2)
            f[j] = jit(f[j], rng.choice([-3, -2, -1, 1, 2, 3]))
        third = a + far() * _dir(np.arctan2(d[1], d[0]) + spread) if rng.randint(0, 2) else a + rng.uniform(-3, 3, 2)
        tri = [a, f, third]
    elif kind == "line":
        j = rng.randint(0, 2)                                                 # on an x = const (0) or y = const (1) line
        near[j] = jit(pm[j] + rng.randint(0, 2), rng.choice([0, 0, -1, 1]))
        near[1 - j] = pm[1 - j] + rng.uniform(0.05, 0.95)
        third = near + far() * _dir(th + spread) if rng.randint(0, 2) else near + rng.uniform(-3, 3, 2)
        tri = [near, near + far() * _dir(th), third]
    elif kind == "axis":
        j = rng.randint(0, 2)                                                 # the long component
        f = near.copy()
        f[j] += rng.choice([-1.0, 1.0]) * far()
        f[1 - j] += rng.choice([-1.0, 1.0]) * AXIS_OFFSETS[rng.randint(0, len(AXIS_OFFSETS))]
        third = near + far() * _dir(th) if rng.randint(0, 2) else near + rng.uniform(-3, 3, 2)
        tri = [near, f, third]
    else:
        raise KeyError(kind)
    return np.array(tri, np.float64).astype(np.float32)


def far_pairs(seed, n, reach, kinds=KINDS, bases=BASES):
    """n (triangle, pixel) pairs, the constructions ``kinds`` in turn, the tested pixel within 16 px of one of ``bases``:
    -> tris (n,3,2) f32, pixmin (n,2) f32, kind (n) index into KINDS."""
    rng = np.random.RandomState(seed)
    tris = np.zeros((n, 3, 2), np.float32); pms = np.zeros((n, 2), np.float32); kind = np.zeros(n, np.int32)
    for i in range(n):
        k = kinds[i % len(kinds)]
        pm = np.floor(bases[rng.randint(0, len(bases))] + rng.uniform(0, 16, 2))
        tris[i] = far_triangle(rng, pm, reach, k)
        pms[i] = pm
        kind[i] = KINDS.index(k)
    return tris, pms, kind


def inside_scene(W, H, seed, n=3, step=0.5):
    """A jittered lattice of faces with the camera inside it: vertices (i, j, k) step for i, j in [-n, n] and k in [-1, 6]
    at world (x, y, z) = (i, j, -k) step, faces the two triangles of every lattice square in the three axis-plane families,
    the camera at the origin looking down -z (scenes.camera shifted by -CAM_DIST, so that view = world and w = -z).
    The lattice plane k = 0 holds the camera: its vertices get |z| < 5e-5 and the projection clamps their |w| to 1e-4, which
    puts them 1e5 .. 1e6 px out; k = -1 is behind the camera; faces that span these planes cross the side of the frustum.
    -> scenes.SoupScene (one camera)."""
    import torch
    from dmesh2_renderer_amd import scenes
    rng = np.random.RandomState(seed)
    ii, jj, kk = np.meshgrid(np.arange(-n, n + 1), np.arange(-n, n + 1), np.arange(-1, 7), indexing="ij")
    ijk = np.stack([ii, jj, kk], -1).reshape(-1, 3)
    xyz = ijk * np.array([step, step, -step]) + rng.uniform(-0.15, 0.15, ijk.shape) * step
    cam_plane = ijk[:, 2] == 0
    xyz[cam_plane, 2] = rng.uniform(-5e-5, 5e-5, cam_plane.sum())
    index = {tuple(p): v for v, p in enumerate(ijk)}
    faces = []
    for (i, j, k) in ijk:
        for u, v in (((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((1, 0, 0), (0, 0, 1))):
            q = [(i, j, k), (i + u[0], j + u[1], k + u[2]), (i + u[0] + v[0], j + u[1] + v[1], k + u[2] + v[2]),
                 (i + v[0], j + v[1], k + v[2])]
            if all(p in index for p in q):
                a, b, c, d = (index[p] for p in q)
                faces += [(a, b, c), (a, c, d)] if rng.randint(0, 2) else [(a, b, d), (b, c, d)]
    P, F = len(xyz), len(faces)
    mv, proj = scenes.camera(W, H, shift=(0.0, 0.0, -scenes.CAM_DIST))
    return scenes.SoupScene(W, H, mv[None], proj[None], torch.from_numpy(xyz.astype(np.float32)),
                            torch.from_numpy(np.array(faces, np.int32)),
                            torch.from_numpy(rng.uniform(0, 1, (P, 3)).astype(np.float32)),
                            torch.from_numpy(rng.uniform(0.3, 0.9, F).astype(np.float32)), torch.ones((1, F)),
                            torch.zeros(3, dtype=torch.float32))


def clip_w(verts, mv, proj):
    """w of the projection (before its |w| clamp), fp64: (B, P)."""
    v = np.asarray(verts, np.float64)
    hom = np.concatenate([v, np.ones_like(v[:, :1])], -1)
    m = np.asarray(mv, np.float64); p = np.asarray(proj, np.float64)
    return np.einsum("pi,bji,bkj->bpk", hom, m, p)[..., 3]
