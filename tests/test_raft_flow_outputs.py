"""RAFT's outputs on the device (ops.flow_to_image / ops.flow_encode_kitti over mpf_flow_to_image / mpf_flow_encode_kitti of mpf_flow_viz.hip;
raft_eval.flow_to_image, save_flow_image, write_flow_kitti, read_flow_kitti; io_formats.png16_from_rgb, read_png_rgb).

golden   tests/golden/flow_viz.npz holds the outputs of the reference's own flow_viz.flow_to_image and frame_utils.writeFlowKITTI (numpy, CPU),
         recorded by tests/golden/make_flow_viz_golden.py.  A missing golden fails.
colours  THE PARITY RULE.  The kernel repeats the reference operation for operation, all of them correctly rounded, except one: the float32
         atan2, whose last bits differ between libraries.  The golden carries per byte `dist`, the distance of the exact (float64) 255 * col
         from the nearest integer.  A byte with dist > DELTA = 0.01 must equal the reference; inside the band it may differ by 1.  DELTA is a
         bound, not a measurement: a few ulp of atan2 (2.4e-7 in a) times 27 in fk times at most 255 levels is about 2e-3 levels, and DELTA
         is five times that.  The recorder gives dist = 0.5 (no band) to every byte the atan2 cannot reach - equal wheel entries, vectors with a
         zero component - and asserts that the band holds at most 5 % of each image; the hand-placed pixels and the all-zero image are exact.
kitti    the code has no transcendental: byte for byte.
"""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "flow_viz.npz")
SYMBOLS = ("mpf_flow_to_image", "mpf_flow_to_image_workspace", "mpf_flow_encode_kitti")
VIZ_CASES = ("rand37x53", "hand5x7", "edge5x7", "zero4x6", "batch2", "clip5", "bgr", "stacked")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ops(built):
    from mpiflow_amd import ops as module
    return module


@pytest.fixture(scope="module")
def raft_eval(built):
    from mpiflow_amd import raft_eval as module
    return module


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN, allow_pickle=False)                  # a missing file is an error here, not a skip
    assert tuple(str(n) for n in z["names"]) == VIZ_CASES and float(z["delta"]) == 0.01
    g = dict(delta=float(z["delta"]), kitti={k: z["kitti9x13/" + k] for k in ("flow", "valid", "code", "code_valid")})
    for name in VIZ_CASES:
        clip = float(z[name + "/clip_flow"])
        g[name] = dict(flow=z[name + "/flow"], image=z[name + "/image"] if name + "/image" in z.files else None, clip_flow=None if clip != clip else clip,
                       convert_to_bgr=bool(z[name + "/convert_to_bgr"]), hand=z[name + "/hand"], out=z[name + "/out"], dist=z[name + "/dist"])
    return g


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def parity(got, case, delta, label):
    """the parity rule; prints the figures before it asserts"""
    ref, dist = case["out"], case["dist"]
    assert got.dtype == np.uint8 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    far = dist > delta
    diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    print("%s: %d bytes, %d in the band; differing: %d outside the band, %d inside, largest difference %d"
          % (label, got.size, int((~far).sum()), int((diff[far] != 0).sum()), int((diff[~far] != 0).sum()), int(diff.max())))
    assert (~far).mean() <= 0.05
    assert (diff[far] == 0).all(), "%s: %d bytes outside the band differ from the reference" % (label, int((diff[far] != 0).sum()))
    assert diff.max() <= 1, "%s: a byte inside the band differs by %d" % (label, int(diff.max()))
    rows = ref.shape[1] - case["flow"].shape[2]              # the stacked form: the colours lie below the frame
    for y, x in case["hand"]:
        assert (got[0, rows + y, x] == ref[0, rows + y, x]).all(), "%s: the hand-placed pixel (%d, %d) differs" % (label, y, x)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("ops", "raft_eval"))
@pytest.mark.parametrize("name", VIZ_CASES)
def test_flow_to_image_matches_the_reference(name, entry, ops, raft_eval, golden):
    case = golden[name]
    flow, image = dev(case["flow"]), dev(case["image"])
    kw = dict(clip_flow=case["clip_flow"], convert_to_bgr=case["convert_to_bgr"])
    if entry == "ops":
        got = ops.flow_to_image(flow, image, **kw)
    elif flow.shape[0] == 1:                                 # upstream's own layout: one [H,W,2] tensor
        got = raft_eval.flow_to_image(flow[0].permute(1, 2, 0), None if image is None else image[0], **kw)[None]
    else:
        got = raft_eval.flow_to_image(flow, image, **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
    parity(got.cpu().numpy(), case, golden["delta"], "%s via %s" % (name, entry))
    if name == "zero4x6":
        assert (got == 255).all()


@pytest.mark.gpu
def test_out_is_written_in_place_and_runs_are_byte_identical(ops, golden):
    case = golden["stacked"]
    flow, image = dev(case["flow"]), dev(case["image"])
    first = ops.flow_to_image(flow, image)
    out = torch.full_like(first, 7)
    assert ops.flow_to_image(flow, image, out=out) is out
    assert torch.equal(out, first) and torch.equal(ops.flow_to_image(flow, image), first)
    k = golden["kitti"]
    code = ops.flow_encode_kitti(dev(k["flow"]), dev(k["valid"]))
    out16 = torch.zeros(code.shape, dtype=torch.int16, device="cuda").view(torch.uint16)
    assert ops.flow_encode_kitti(dev(k["flow"]), dev(k["valid"]), out=out16) is out16 and torch.equal(out16.view(torch.int16), code.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("stacked", (False, True))
def test_a_batch_equals_its_images_one_by_one(stacked, ops, golden):
    """three 37 x 53 images with rad_max 700 x apart: 1961 pixels each (3922 stacked), so images begin and end inside blocks of 1024 pixels,
    and neither the pixel count nor the byte count of an image is a multiple of 4"""
    base = golden["rand37x53"]["flow"][0]
    flow = dev(np.stack([base, base * np.float32(0.01), base[:, ::-1] * np.float32(7)]))
    image = torch.rand(3, 3, 37, 53, device="cuda") * 255 if stacked else None
    for bgr in (False, True):
        whole = ops.flow_to_image(flow, image, convert_to_bgr=bgr)
        assert whole.shape == (3, 74 if stacked else 37, 53, 3)
        for n in range(3):
            assert torch.equal(whole[n:n + 1], ops.flow_to_image(flow[n:n + 1], None if image is None else image[n:n + 1], convert_to_bgr=bgr)), (n, bgr)
    rgb = ops.flow_to_image(flow, image)
    assert torch.equal(rgb.flip(-1), whole)                  # convert_to_bgr reverses the channels of both halves
    if stacked:
        assert torch.equal(rgb[:, :37], image.permute(0, 2, 3, 1).to(torch.uint8))
        assert torch.equal(rgb[:, 37:], ops.flow_to_image(flow))


@pytest.mark.gpu
def test_rad_max_sees_every_pixel_of_a_large_image(ops):
    """260 x 260 = 67600 pixels: more than 256 blocks of 256, so the maximum's blocks stride; the largest vector sits at the last pixel"""
    g = torch.Generator().manual_seed(9130)
    a = torch.randn(1, 2, 260, 260, generator=g)
    a[0, :, -1, -1] = torch.tensor([300.0, -400.0])
    b = a.clone()
    b[0, :, 0, 0] = torch.tensor([-300.0, 400.0])            # the same rad_max, found by the first block
    ia, ib = ops.flow_to_image(a.cuda()), ops.flow_to_image(b.cuda())
    assert torch.equal(ia.reshape(-1, 3)[1:], ib.reshape(-1, 3)[1:])
    assert (ia[0, :-1] >= 250).float().mean() > 0.99         # noise of 1 px under a maximum of 500 px: almost white


@pytest.mark.gpu
def test_kitti_code_is_the_reference_code_byte_for_byte(ops, golden):
    k = golden["kitti"]
    for valid, want in ((None, k["code"]), (k["valid"], k["code_valid"])):
        got = ops.flow_encode_kitti(dev(k["flow"]), dev(valid))
        assert got.dtype == torch.uint16 and got.shape == (1, 9, 13, 3) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
    two = ops.flow_encode_kitti(dev(np.concatenate([k["flow"], -k["flow"][:, :, ::-1]])))         # 2 x 117 pixels: an odd count per image
    assert np.array_equal(two[0].cpu().numpy(), k["code"][0]) and torch.equal(two[1:].view(torch.int16), ops.flow_encode_kitti(dev(-k["flow"][:, :, ::-1])).view(torch.int16))


@pytest.mark.gpu
def test_kitti_code_clamps_outside_512_px(ops):
    flow = torch.tensor([[[[600.0, -600.0, 511.984375]], [[-512.0, 512.0, float("nan")]]]]).cuda()           # [1,2,1,3]
    got = ops.flow_encode_kitti(flow).cpu().numpy().astype(np.int64)
    assert got.tolist() == [[[[65535, 0, 1], [0, 65535, 1], [65535, 0, 1]]]]


@pytest.mark.gpu
def test_write_flow_kitti_round_trips(raft_eval, golden, tmp_path):
    k = golden["kitti"]
    path = str(tmp_path / "000000_10.png")
    raft_eval.write_flow_kitti(path, dev(k["flow"][0]), dev(k["valid"][0]))
    flow, valid = raft_eval.read_flow_kitti(path)
    assert flow.shape == (9, 13, 2) and flow.dtype == np.float32 and np.array_equal(valid, k["valid"][0])
    err = np.abs(flow - k["flow"][0].transpose(1, 2, 0)).max()
    print("round trip: max |flow - read| = %.6f px (bound 1/64 = %.6f)" % (err, 1 / 64))
    assert err <= 1 / 64
    raft_eval.write_flow_kitti(path, dev(k["flow"]))         # [1,2,H,W], no valid: all ones
    assert (raft_eval.read_flow_kitti(path)[1] == 1).all()
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:                             # another decoder agrees about the size (Pillow has no 16-bit RGB mode to compare samples)
        assert im.size == (13, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("stacked", (False, True))
def test_save_flow_image_holds_the_kernels_bytes(stacked, ops, raft_eval, golden, tmp_path):
    case = golden["stacked"]
    flow, image = dev(case["flow"]), dev(case["image"]) if stacked else None
    path = str(tmp_path / "flow.png")
    raft_eval.save_flow_image(path, flow[0], None if image is None else image[0])
    want = ops.flow_to_image(flow, image)[0].cpu().numpy()   # R, G, B, as the file holds it
    try:
        from PIL import Image
        with Image.open(path) as im:
            got = np.asarray(im.convert("RGB"))
    except ImportError:
        from mpiflow_amd import io_formats
        got = io_formats.read_png_rgb(path)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_the_new_symbols(built):
    hdr = open(os.path.join(ROOT, "include", "mpiflow_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in built.SIGNATURES and hasattr(built.load(), s), s
    assert "MpfFlowVizArgs" in hdr and ctypes.sizeof(built.MpfFlowVizArgs) == 72
    lib = built.load()
    assert lib.mpf_flow_to_image(None, None) == 10001 and b"null argument block" in lib.mpf_last_error()
    assert lib.mpf_flow_encode_kitti(None, None) == 10001
    assert lib.mpf_flow_to_image_workspace(1, 436, 1024) == 256 * 4 and lib.mpf_flow_to_image_workspace(2, 5, 7) == 2 * 4
    assert lib.mpf_flow_to_image_workspace(0, 5, 7) == 0 and lib.mpf_flow_to_image_workspace(4, 20000, 20000) == 0
    a = built.MpfFlowVizArgs()
    a.N, a.H, a.W, a.flow, a.out = 1, 4, 4, 256, 258
    assert lib.mpf_flow_to_image(ctypes.byref(a), None) == 10001 and b"out must be 4-byte aligned" in lib.mpf_last_error()
    a.out = 256
    assert lib.mpf_flow_to_image(ctypes.byref(a), None) == 10001 and b"workspace" in lib.mpf_last_error()


def test_refusals_name_the_fault_and_judge_the_device_last(built):
    from mpiflow_amd import ops, raft_eval
    E = built.MpiFlowHipError
    z = torch.zeros
    for call in (ops.flow_to_image, ops.flow_encode_kitti, raft_eval.flow_to_image):
        who = call.__name__
        with pytest.raises(E, match=who + r": flow must be a torch\.Tensor \(got list\)"):
            call([1, 2])
        for dtype in (torch.float16, torch.float64):
            with pytest.raises(E, match=who + r": flow must be float32 \(got %s\).*\.float\(\)" % str(dtype).replace(".", r"\.")):
                call(z(1, 2, 4, 6, dtype=dtype))
        with pytest.raises(E, match=who + r": flow must be \[N,2,H,W\], a contiguous tensor of 4 dimensions \(got shape \(1, 3, 4, 6\)\)"):
            call(z(1, 3, 4, 6))
        with pytest.raises(E, match=who + r": flow must be contiguous \(got shape"):
            call(z(1, 2, 6, 4).transpose(2, 3))
        with pytest.raises(E, match=who + r": flow must live on the GPU \(got cpu\); mpiflow_amd has no CPU path"):
            call(z(1, 2, 4, 6))
    with pytest.raises(E, match=r"flow_to_image: image must be \[N,3,H,W\] like flow, a contiguous tensor of 4 dimensions \(got shape \(1, 3, 4, 8\)\)"):
        ops.flow_to_image(z(1, 2, 4, 6), z(1, 3, 4, 8))
    with pytest.raises(E, match=r"flow_to_image: image must be float32 \(got torch\.uint8\).*\.float\(\)"):
        ops.flow_to_image(z(1, 2, 4, 6), z(1, 3, 4, 6, dtype=torch.uint8))
    with pytest.raises(E, match=r"flow_to_image: out must be uint8 \(got torch\.float32\)"):
        ops.flow_to_image(z(1, 2, 4, 6), out=z(1, 4, 6, 3))
    with pytest.raises(E, match=r"flow_to_image: out must be \[N,2H,W,3\], a contiguous tensor of 4 dimensions \(got shape \(1, 4, 6, 3\)\)"):
        ops.flow_to_image(z(1, 2, 4, 6), z(1, 3, 4, 6), out=z(1, 4, 6, 3, dtype=torch.uint8))
    with pytest.raises(E, match=r"flow_to_image: out must be 4-byte aligned"):
        ops.flow_to_image(z(1, 2, 4, 6), out=z(1 + 4 * 6 * 3, dtype=torch.uint8)[1:].view(1, 4, 6, 3))
    with pytest.raises(E, match=r"flow_to_image: clip_flow must be None or a number \(got 'all'\)"):
        ops.flow_to_image(z(1, 2, 4, 6), clip_flow="all")
    with pytest.raises(E, match=r"flow_to_image: flow must have at least one image and one pixel"):
        ops.flow_to_image(z(0, 2, 4, 6))
    with pytest.raises(E, match=r"flow_encode_kitti: valid must be \[N,H,W\] like flow, a contiguous tensor of 3 dimensions \(got shape \(1, 1, 4, 6\)\)"):
        ops.flow_encode_kitti(z(1, 2, 4, 6), z(1, 1, 4, 6))
    with pytest.raises(E, match=r"flow_encode_kitti: out must be uint16 \(got torch\.int16\)"):
        ops.flow_encode_kitti(z(1, 2, 4, 6), out=z(1, 4, 6, 3, dtype=torch.int16))
    with pytest.raises(E, match=r"flow_to_image: flow must be \[N,2,H,W\] or \[H,W,2\] \(got shape \(2, 4, 6\)\)"):
        raft_eval.flow_to_image(z(2, 4, 6))
    with pytest.raises(E, match=r"write_flow_kitti: one file holds one image: flow must be a single sample \(got shape \(2, 2, 4, 6\)\)"):
        raft_eval.write_flow_kitti("unused.png", z(2, 2, 4, 6))
    with pytest.raises(E, match=r"flow_to_image: flow must live on the GPU"):        # the device last: everything else about the call is in order
        raft_eval.save_flow_image("unused.png", z(2, 4, 6), z(3, 4, 6))


def test_png16_header_and_sample_order():
    from mpiflow_amd import io_formats
    img = np.array([[[0x0102, 0x8000, 1], [65535, 0, 0x00FF]], [[0x0203, 0x8001, 0], [3, 2, 1]]], np.uint16)
    data = io_formats.png16_from_rgb(img)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    assert data[8:16] == struct.pack(">I", 13) + b"IHDR"
    assert struct.unpack(">IIBBBBB", data[16:29]) == (2, 2, 16, 2, 0, 0, 0)          # 2 x 2, bit depth 16, colour type 2 (RGB), no interlace
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT" and data[-12:-8] == struct.pack(">I", 0) and data[-8:-4] == b"IEND"
    rows = np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(2, 13)
    assert rows[:, 0].tolist() == [2, 2]                     # filter "Up"
    first = rows[0, 1:]
    assert first.tolist() == [0x01, 0x02, 0x80, 0x00, 0x00, 0x01, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0xFF]       # most significant byte first
    assert ((rows[1, 1:].astype(np.int64) + first) % 256).tolist() == [0x02, 0x03, 0x80, 0x01, 0, 0, 0, 3, 0, 2, 0, 1]
    back = io_formats.read_png_rgb(data)
    assert back.dtype == np.uint16 and np.array_equal(back, img)
    with pytest.raises(AssertionError):
        io_formats.png16_from_rgb(img.astype(np.uint8))


def test_read_png_rgb_inverts_every_row_filter(tmp_path):
    from mpiflow_amd import io_formats
    rng = np.random.default_rng(9140)
    img = rng.integers(0, 256, (7, 5, 3), dtype=np.uint8)
    assert np.array_equal(io_formats.read_png_rgb(io_formats.png_from_scanlines(io_formats.filter_up_rgb(img))), img)
    flat = img.reshape(7, 15).astype(np.int64)
    rows = []
    for y in range(7):                                       # filters 0 .. 4, written out from the PNG specification
        ft = y % 5
        cur, up = flat[y], flat[y - 1] if y else np.zeros(15, np.int64)
        left, upleft = np.concatenate([np.zeros(3, np.int64), cur[:-3]]), np.concatenate([np.zeros(3, np.int64), up[:-3]])
        p = left + up - upleft
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        pred = (np.zeros(15, np.int64), left, up, (left + up) // 2, paeth)[ft]
        rows.append(bytes([ft]) + ((cur - pred) % 256).astype(np.uint8).tobytes())
    chunk = io_formats._png_chunk
    data = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 7, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(b"".join(rows)))
            + chunk(b"IEND", b""))
    path = tmp_path / "filters.png"
    path.write_bytes(data)
    assert np.array_equal(io_formats.read_png_rgb(str(path)), img)
    with pytest.raises(ValueError, match="not a PNG"):
        io_formats.read_png_rgb(b"GIF89a..")
