"""Per-face blend weights of the layer compositor, restated in float64 (the contract of dm2_layers_composite's out_face_weights).

face_weights[b, f] = sum over the pixels of view b and the layers that blend (the float32 decisions of
layer_composite_ref.forward32) of faces_opacity[f] * T, with T the product of (1 - alpha) of the layers that blended in front
of it in the same pixel.  A face listed twice in one pixel counts twice.
"""
import numpy as np


def layered_face_weights64(fwd, faces_opacity, F):
    """fwd: layer_composite_ref.forward32(...) -> (B, F) float64."""
    blend, fs = fwd["blend"], fwd["fs"]
    B, H, W, L = blend.shape
    op = np.asarray(faces_opacity, dtype=np.float64)
    out = np.zeros((B, F), np.float64)
    if F == 0:
        return out
    T = np.ones((B, H, W), np.float64)
    bidx = np.broadcast_to(np.arange(B).reshape(B, 1, 1), (B, H, W))
    for l in range(L):
        act = blend[..., l]
        a = op[fs[..., l]]
        np.add.at(out, (bidx[act], fs[..., l][act]), (a * T)[act])
        T = np.where(act, T * (1.0 - a), T)
    return out
