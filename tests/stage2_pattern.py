"""Closed-form weights and inputs for the EdgeConnect generators' numerics golden (tests/golden/stage2.npz): the maker fills the REFERENCE's
generators with pattern_state_dict and records their outputs; the test fills the project's generators with the same function, so no weights
file is committed.  Nothing here draws from a random generator.

The value at flat index i of the k-th key in sorted order is a_k sin(0.37 i + k + 0.001 i^2), formed in float64 and rounded once.  The
quadratic term keeps a layer's output channels from all lying in the plane spanned by one sine and one cosine.  a_k: 1 / sqrt(fan_in) for a
convolution weight (so every layer's output is O(1) whatever follows it), 0.1 for a bias, and for the weight_u / weight_v of spectral norm
the reciprocal of the pattern's own 2-norm, unit vectors as a checkpoint holds them."""
import numpy as np

GENERATORS = ("edge", "inpaint", "disp")
SIZE = 32                        # 8 x 8 at the bottleneck: enough for the reflection pad of the dilation-2 blocks


def build(module, name):
    """one of the three generators as get_edge_connect constructs them, from `module` (the reference's networks.py or the project's)"""
    if name == "edge":
        return module.EdgeGenerator()
    if name == "inpaint":
        return module.InpaintGenerator()
    return module.InpaintGenerator(in_channels=2, out_channels=1)


def pattern(n, k):
    i = np.arange(n, dtype=np.float64)
    return np.sin(0.37 * i + k + 0.001 * i * i)


def pattern_state_dict(shapes):
    """shapes: {key: shape} -> {key: float32 array}"""
    out = {}
    for k, key in enumerate(sorted(shapes)):
        shape = tuple(shapes[key])
        n = int(np.prod(shape)) if shape else 1
        v = pattern(n, k)
        if key.endswith("weight_u") or key.endswith("weight_v"):
            a = 1.0 / np.sqrt(np.sum(v * v))
        elif key.endswith("bias"):
            a = 0.1
        else:
            a = 1.0 / np.sqrt(n / shape[0])
        out[key] = (a * v).reshape(shape).astype(np.float32)
    return out


def load_pattern(model):
    """fills a generator's state dict with the pattern (strict) and puts it in eval mode; returns the model"""
    import torch
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in pattern_state_dict(shapes).items()}, strict=True)
    return model.eval()


def golden_input(name):
    """[1,C,32,32] float32 in [0, 1]: the edge generator gets (gray, 0/1 edges, 0/1 hole), the others (image or disparity + hole, edges)"""
    c = {"edge": 3, "inpaint": 4, "disp": 2}[name]
    x = 0.5 + 0.5 * pattern(c * SIZE * SIZE, 100 + c).reshape(1, c, SIZE, SIZE)
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    hole = ((yy - 14) ** 2 + (xx - 18) ** 2 < 49).astype(np.float64)
    if name == "edge":
        x[0, 1] = x[0, 1] > 0.9
        x[0, 2] = hole
    else:
        x[0, :-1] += hole
    return x.astype(np.float32)
