"""The tensor contract of the RAFT modules (mpiflow_amd/_tensors.py): type, float32, shape, contiguity per tensor in that order, whatever the
call itself requires, the device last.  Host only: every refusal here is raised before the library is loaded, and `no_library` makes sure."""
import itertools

import pytest
import torch

from mpiflow_amd import _lib, _tensors
from mpiflow_amd._tensors import check_devices, check_pyramid, check_tensor

E = _lib.MpiFlowHipError

# the four faults of one tensor in the order they are judged: (what turns a good [2,3,4,5] tensor into a faulty one, the words that name the fault)
FAULTS = (("type", lambda t: t.numpy(), r"x must be a torch\.Tensor \(got ndarray\)"),
          ("dtype", lambda t: t.double(), r"x must be float32 \(got torch\.float64\)"),
          ("shape", lambda t: t[:, :, :3].contiguous(), r"x must be \[N,C,H,W\], .* 4 dimensions \(got shape \(2, 3, 3, 5\)\)"),
          ("contiguous", lambda t: t.transpose(2, 3).contiguous().transpose(2, 3), r"x must be contiguous"))
SHAPE = (2, 3, 4, None)


@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise AssertionError("the library was asked for before the arguments were judged")
    monkeypatch.setattr(_lib, "load", load)


def test_the_contract_is_three_functions_and_cannot_load_the_library():
    names = {n for n in vars(_tensors) if not n.startswith("__")}
    assert names == {"torch", "CORR_MAX_LEVELS", "MpiFlowHipError", "check_tensor", "check_devices", "check_pyramid"}


def test_a_good_tensor_comes_back_as_it_is():
    t = torch.zeros(2, 3, 4, 5)
    assert check_tensor(t, "x", "who", SHAPE, "[N,C,H,W]") is t
    assert check_tensor(t, "x", "who", 4) is t
    assert check_tensor(t, "x", "who", (None, None, None, None)) is t                # a free entry takes any size
    for n in (1, 7):
        u = torch.zeros(2, 3, 4, n)
        assert check_tensor(u, "x", "who", SHAPE) is u
    s = torch.zeros(())
    assert check_tensor(s, "g", "who", ()) is s and check_tensor(s, "g", "who", 0) is s


@pytest.mark.parametrize("fault", FAULTS, ids=[f[0] for f in FAULTS])
def test_each_fault_alone_is_named(fault):
    _, spoil, words = fault
    with pytest.raises(E, match="who: " + words):
        check_tensor(spoil(torch.zeros(2, 3, 4, 5)), "x", "who", SHAPE, "[N,C,H,W]")


def test_shape_faults_of_every_kind():
    for bad in (torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, 5, 1), torch.zeros(1, 3, 4, 5), torch.zeros(2, 3, 5, 5)):
        with pytest.raises(E, match=r"x must be \[2, 3, 4, None\], a contiguous tensor of 4 dimensions \(got shape"):
            check_tensor(bad, "x", "who", SHAPE)
    with pytest.raises(E, match=r"who: x must be a contiguous tensor of 3 dimensions \(got shape \(2, 3, 4, 5\)\)"):
        check_tensor(torch.zeros(2, 3, 4, 5), "x", "who", 3)


@pytest.mark.parametrize("first,second", list(itertools.combinations(range(1, 4), 2)), ids=lambda i: FAULTS[i][0])
def test_of_two_faults_the_earlier_one_is_named(first, second):
    """dtype < shape < contiguity (a non-tensor has no second fault to show)"""
    t = FAULTS[second][1](FAULTS[first][1](torch.zeros(2, 3, 4, 5)))
    assert [i for i in (1, 2, 3) if faulty(t, i)] == [first, second]
    with pytest.raises(E, match=FAULTS[first][2]):
        check_tensor(t, "x", "who", SHAPE, "[N,C,H,W]")


def faulty(t, i):
    return (t.dtype != torch.float32, tuple(t.shape[:3]) != (2, 3, 4), not t.is_contiguous())[i - 1]


def test_all_three_faults_name_the_dtype_and_a_non_tensor_its_type():
    t = FAULTS[3][1](FAULTS[2][1](torch.zeros(2, 3, 4, 5))).double()
    assert all(faulty(t, i) for i in (1, 2, 3))
    with pytest.raises(E, match="x must be float32"):
        check_tensor(t, "x", "who", SHAPE)
    with pytest.raises(E, match=r"x must be a torch\.Tensor \(got list\)"):
        check_tensor([t], "x", "who", SHAPE)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16, torch.float64, torch.int32))
def test_another_dtype_is_told_to_call_float(dtype):
    with pytest.raises(E, match=r"who: mask must be float32 \(got %s\).*\.float\(\)" % str(dtype).replace(".", r"\.")):
        check_tensor(torch.zeros(2, 3, 4, 5, dtype=dtype), "mask", "who", 4)


def test_device_check():
    check_devices("who", {})
    a, b = torch.zeros(3), torch.zeros(3)
    with pytest.raises(E, match=r"who: a must live on the GPU \(got cpu\); mpiflow_amd has no CPU path"):
        check_devices("who", dict(a=a, b=b))
    with pytest.raises(E, match=r"who: levels\[1\] must live on the GPU.*no CPU path"):
        check_devices("who", {"levels[1]": b})
    # the other sentence ("... must share one device") needs tensors on two GPUs; the gpu tests of the five modules run check_devices with live
    # buffers (test_gpu_tensors_that_disagree_are_refused_and_nothing_is_launched), and no device is faked here


def test_pyramid_geometry():
    L = _lib.CORR_MAX_LEVELS
    check_pyramid("who", 16, 16, 4, 4)
    check_pyramid("who", 16, 16, 4)
    check_pyramid("who", 2, 2, 1, 1)
    check_pyramid("who", 2 ** L, 2 ** L, L, 8)
    check_pyramid("who", None, None, L)
    for levels in (0, L + 1):
        with pytest.raises(E, match=r"who: num_levels must be 1\.\.%d \(got %d\)" % (L, levels)):
            check_pyramid("who", 1024, 1024, levels, 4)
        with pytest.raises(E, match="num_levels must be 1.."):
            check_pyramid("who", None, None, levels)
    for radius in (0, 9):
        with pytest.raises(E, match=r"who: radius must be 1\.\.8 \(got %d\)" % radius):
            check_pyramid("who", 16, 16, 4, radius)
    for H, W in ((15, 24), (16, 15)):
        with pytest.raises(E, match=r"who: H, W = %d, %d must be at least 2\^num_levels = 16" % (H, W)):
            check_pyramid("who", H, W, 4, 4)
    with pytest.raises(E, match="num_levels must be 1.."):                            # of two faults: the levels, the radius, the frame
        check_pyramid("who", 1, 1, 0, 0)
    with pytest.raises(E, match="radius must be 1.."):
        check_pyramid("who", 1, 1, 4, 0)


def entry_points():
    """(name, call(tensor)) for one entry point of each family: the call hands `tensor` where a float32 [2,32,16,16] tensor is expected, with
    everything else in order but on the CPU"""
    from mpiflow_amd import ops, raft_corr, raft_extractor, raft_update
    z = torch.zeros
    nhwc = lambda: z(2, 16, 16, 32)
    levels = lambda: [z(2 * 256, 16 >> i, 16 >> i) for i in range(4)]
    gru = raft_update.SepConvGRU(hidden_dim=32, input_dim=8)
    block = raft_extractor.ResidualBlock(32, 32, "instance")
    return [("ops.corr_lookup", lambda t: ops.corr_lookup(nhwc(), [t], z(2, 2, 16, 16), 4), "f2_levels_nhwc\\[0\\]"),
            ("ops.corr_volume_lookup", lambda t: ops.corr_volume_lookup(levels(), t, 4), "coords"),
            ("ops.upsample_flow", lambda t: ops.upsample_flow(z(2, 2, 16, 16), t), "mask"),
            ("ops.gru_reset", lambda t: ops.gru_reset(t, [(z(2, 64, 16, 16), 0)]), "h"),
            ("ops.norm_act", lambda t: ops.norm_act(ops.NormTerm(t, "instance")), "term.x"),
            ("AlternateCorrBlock", lambda t: raft_corr.AlternateCorrBlock(z(2, 32, 16, 16), t), "fmap2"),
            ("CorrBlock", lambda t: raft_corr.CorrBlock(t, z(2, 32, 16, 16)), "fmap1"),
            ("SepConvGRU", lambda t: gru(t, z(2, 8, 16, 16)), "h"),
            ("ResidualBlock", lambda t: block(t), "x")]


ENTRY_POINTS = ("ops.corr_lookup", "ops.corr_volume_lookup", "ops.upsample_flow", "ops.gru_reset", "ops.norm_act", "AlternateCorrBlock", "CorrBlock",
                "SepConvGRU", "ResidualBlock")


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_the_device_is_judged_last_in_every_family(entry, no_library):
    """a CPU tensor that is also of the wrong dtype, or of the wrong shape, is told about the dtype or the shape; one that is only on the CPU,
    about the device"""
    cases = {c[0]: c for c in entry_points()}
    assert tuple(cases) == ENTRY_POINTS
    _, call, name = cases[entry]
    with pytest.raises(E, match=name + r" must be float32 \(got torch\.float16\).*\.float\(\)"):
        call(torch.zeros(2, 32, 16, 16, dtype=torch.float16))
    with pytest.raises(E, match=name + r" must be .*dimensions \(got shape \(32, 16, 16\)\)"):
        call(torch.zeros(32, 16, 16))
    good = {"ops.corr_lookup": (2, 16, 16, 32), "ops.corr_volume_lookup": (2, 2, 16, 16), "ops.upsample_flow": (2, 576, 16, 16)}.get(entry, (2, 32, 16, 16))
    with pytest.raises(E, match="no CPU path"):
        call(torch.zeros(good))
