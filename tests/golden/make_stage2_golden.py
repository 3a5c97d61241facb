#!/usr/bin/env python3
"""Record the EdgeConnect generators of warp-back stage 2 by RUNNING THE REFERENCE ITSELF (warpback/networks.py, which needs only torch) on
the CPU -> tests/golden/edgeconnect_keys.json and tests/golden/stage2.npz.

    python tests/golden/make_stage2_golden.py [--out-dir DIR]   (in the build container: needs the reference tree, numpy, torch)

edgeconnect_keys.json   the state-dict keys and shapes of the three generators as get_edge_connect constructs them: names and numbers only.
stage2.npz              per generator, filled with the closed-form weights of tests/stage2_pattern.py (no weights are stored): the golden
                        input [1,C,32,32], the reference's float32 output and its float64 output with the module cast to double.

The EdgeConnect checkpoints are installed nowhere: what real weights give is unpinned.  The recorder asserts that
each output is spread over (0, 1), not saturated, so that a wrong pad or dilation cannot hide behind a flat sigmoid."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import stage2_pattern as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=HERE)
    a = ap.parse_args()
    import torch
    sys.path.insert(0, HERE)
    import ref_harness
    ref_harness.install()
    from warpback import networks as ref        # the reference's own

    keys, rec = {}, {"torch_version": np.array(torch.__version__)}
    for name in P.GENERATORS:
        model = P.build(ref, name)
        keys[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
        P.load_pattern(model)
        x = torch.from_numpy(P.golden_input(name))
        with torch.no_grad():
            y32 = model(x).numpy()
            y64 = model.double()(x.double()).numpy()
        spread = float(((y64 > 0.02) & (y64 < 0.98)).mean())
        e_ref = float(np.abs(y32 - y64).max())
        print("%-8s out %s  mean %.3f std %.3f  share in (0.02, 0.98) %.2f  e_ref = max|ref32 - ref64| = %.3e" % (name, y32.shape, y64.mean(), y64.std(), spread, e_ref))
        assert y64.std() > 0.05 and spread > 0.5, (name, y64.std(), spread)
        rec["%s_in" % name], rec["%s_ref32" % name], rec["%s_ref64" % name] = x.numpy(), y32, y64
    with open(os.path.join(a.out_dir, "edgeconnect_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write("\n")
    out = os.path.join(a.out_dir, "stage2.npz")
    np.savez_compressed(out, **rec)
    print("wrote %s, %d bytes" % (out, os.path.getsize(out)))
    assert os.path.getsize(out) < 200 * 1000
    return 0


if __name__ == "__main__":
    sys.exit(main())
