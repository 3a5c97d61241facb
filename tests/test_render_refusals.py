"""CPU-only: every bad-argument call of the render launchers (mpf_render.hip) comes back as MPF_ERR_BAD_ARGUMENT with exactly the message below, before
anything is launched - so no device is needed, and the pointers are fakes that are never dereferenced.  The table pins the wording of every check and, with
the two-fault rows, the order in which each entry point judges them."""
import ctypes

import pytest

ONE = ctypes.c_void_p(256)          # an aligned fake device pointer
ODD = ctypes.c_void_p(260)          # a misaligned one
S, H, W = 4, 8, 8
N = H * W


def A(k):
    """distinct 16-byte aligned fake buffers, 64 KiB apart: further than any buffer of an S x H x W call is long"""
    return 0x10000 * k


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from mpiflow_amd import _lib
    return _lib


def sbf(lib, L, entry="mpf_src_blend_flow", mpi=ONE, img=ONE, params=ONE, P=0, S=S, H=H, W=W, rgba=None, flows=None, obj_mask=None, quads=None, quads_c=None,
        sup=None, sup_c=None):
    args = [mpi, img, params, P, S, H, W, 0.0, rgba, None, None, flows, None, obj_mask, quads, quads_c, None]
    if entry.endswith("_support"):
        args += [sup, sup_c, 1]
    return getattr(lib, entry)(*args, None)


def view(L, **kw):
    f = dict(d_params=256, d_rgb=A(8))
    f.update(kw)
    return L.MpfWarpView(**f)


MASKED = dict(d_mask_quads=A(9), d_objmask=A(10))


def _views(L, vs, n):
    vs = [view(L)] if vs is None else [view(L, **v) for v in vs]
    return (L.MpfWarpView * 17)(*vs), (len(vs) if n is None else n)


def _supports(L, cells):
    return None if cells is None else (L.MpfViewSupport * 17)(*[L.MpfViewSupport(c, 1, 0.5) for c in cells])


def wcv(lib, L, entry="mpf_warp_composite_views", rgba=ONE, inter=2, vs=None, n=None, S=S, H=H, W=W, cells=None):
    arr, n = _views(L, vs, n)
    if entry.endswith("_support"):
        return getattr(lib, entry)(rgba, inter, arr, _supports(L, cells), n, S, H, W, None)
    return getattr(lib, entry)(rgba, inter, arr, n, S, H, W, None)


def merge(L, **kw):
    f = dict(d_frame=A(20), d_frame_dyn=A(21), d_mask=A(22), d_mask_dyn=A(23), d_flow=A(24), d_flow_dyn=A(25), d_obj_mask=A(26), thresh=0.99,
             d_flow_mix=A(27), d_frame_mix=A(28), d_fill_mask=A(29), obj_mask_stride=1)
    f.update(kw)
    return L.MpfMergeArgs(**f)


NEXT, MERGE, MERGE_SUP = "mpf_warp_views_and_blend_next", "mpf_warp_views_blend_next_merge_prev", "mpf_warp_views_blend_next_merge_prev_support"


def pair(lib, L, entry=NEXT, rgba=A(1), vs=None, n=None, mpi=ONE, img=ONE, params=ONE, P=0, out=A(2), flows=None, src_u8=None, obj_mask=None, quads=None,
         quads_c=None, S=S, H=H, W=W, mg=None, cells=None, sup=None, sup_c=None):
    arr, n = _views(L, vs, n)
    head = [rgba, arr] + ([_supports(L, cells)] if entry == MERGE_SUP else []) + [n]
    next_ = [mpi, img, params, P, 0.0, out, flows, src_u8, obj_mask, quads, quads_c, None] + ([sup, sup_c, 1] if entry == MERGE_SUP else [])
    tail = [] if entry == NEXT else [ctypes.byref(merge(L, **mg)) if mg is not None else None]
    return getattr(lib, entry)(*head, *next_, S, H, W, *tail, None)


SBF = "mpf_src_blend_flow: "                           # both Stage A+C entries name this one
WCV = "mpf_warp_composite_views: "
PAIR = "mpf_warp_views_and_blend_next: "                # the pair launch names this entry whichever wrapper was called
MP = "mpf_warp_views_blend_next_merge_prev: "
GIB = PAIR + "the plane stack must be smaller than 4 GiB (buffer addressing); use the two separate calls"
P_PAIR = PAIR + "P must be 0..2, flows output iff P > 0"
FLOWS = MP + "merge_prev's flows must be disjoint from d_flows_next or exactly its two pose planes"
OBJ = MP + "merge_prev's object mask must not be a buffer this launch writes (other than the .x of d_quads_next, stride 4)"

ROWS = [
    # ---- Stage A+C alone ----------------------------------------------------------------------------------------------------------------------------------
    ("sbf-P3", lambda lib, L: sbf(lib, L, P=3, flows=ONE), SBF + "P must be 0, 1 or 2 (got 3)"),
    ("sbf-flows-with-P0", lambda lib, L: sbf(lib, L, flows=ONE), SBF + "flows output iff P > 0"),
    ("sbf-P2-without-flows", lambda lib, L: sbf(lib, L, P=2), SBF + "flows output iff P > 0"),
    ("sbf-quads-without-mask", lambda lib, L: sbf(lib, L, quads=ONE), SBF + "quads need d_obj_mask"),
    ("sbf-complement-quads-without-mask", lambda lib, L: sbf(lib, L, quads_c=ONE), SBF + "quads need d_obj_mask"),
    ("sbf-misaligned-quads", lambda lib, L: sbf(lib, L, obj_mask=ONE, quads=ODD), SBF + "quads must be 16-byte aligned"),
    ("sbf-misaligned-complement-quads", lambda lib, L: sbf(lib, L, obj_mask=ONE, quads=ONE, quads_c=ODD), SBF + "quads must be 16-byte aligned"),
    ("sbf-support-without-quads", lambda lib, L: sbf(lib, L, "mpf_src_blend_flow_support", sup=ONE), SBF + "a support map needs its quads"),
    ("sbf-complement-support-without-quads", lambda lib, L: sbf(lib, L, "mpf_src_blend_flow_support", obj_mask=ONE, quads=ONE, sup=ONE, sup_c=ONE),
     SBF + "a support map needs its quads"),
    ("sbf-S5000", lambda lib, L: sbf(lib, L, S=5000), SBF + "bad shape S=5000 H=8 W=8"),
    ("sbf-W0", lambda lib, L: sbf(lib, L, W=0), SBF + "bad shape S=4 H=8 W=0"),
    ("sbf-null", lambda lib, L: sbf(lib, L, img=None), SBF + "null pointer"),
    ("sbf-misaligned-rgba", lambda lib, L: sbf(lib, L, rgba=ODD), SBF + "rgba output must be 16-byte aligned"),
    ("sbf-support-entry-P3", lambda lib, L: sbf(lib, L, "mpf_src_blend_flow_support", P=3, flows=ONE), SBF + "P must be 0, 1 or 2 (got 3)"),
    ("sbf-support-entry-S5000", lambda lib, L: sbf(lib, L, "mpf_src_blend_flow_support", S=5000), SBF + "bad shape S=5000 H=8 W=8"),
    # two faults: which one is reported
    ("sbf-support-before-null", lambda lib, L: sbf(lib, L, "mpf_src_blend_flow_support", mpi=None, sup=ONE), SBF + "a support map needs its quads"),
    ("sbf-null-before-quads", lambda lib, L: sbf(lib, L, mpi=None, quads=ONE), SBF + "null pointer"),
    ("sbf-mask-before-alignment", lambda lib, L: sbf(lib, L, quads=ODD), SBF + "quads need d_obj_mask"),
    ("sbf-alignment-before-P", lambda lib, L: sbf(lib, L, P=3, obj_mask=ONE, quads=ODD), SBF + "quads must be 16-byte aligned"),
    ("sbf-P-before-flows", lambda lib, L: sbf(lib, L, P=-1), SBF + "P must be 0, 1 or 2 (got -1)"),
    ("sbf-flows-before-shape", lambda lib, L: sbf(lib, L, flows=ONE, S=5000), SBF + "flows output iff P > 0"),
    ("sbf-shape-before-rgba", lambda lib, L: sbf(lib, L, S=0, rgba=ODD), SBF + "bad shape S=0 H=8 W=8"),
    # ---- the flow-only pass -------------------------------------------------------------------------------------------------------------------------------
    ("flow-null", lambda lib, L: lib.mpf_src_flow(ONE, ONE, 1, S, H, W, 0.0, None, None), "mpf_src_flow: null pointer"),
    ("flow-P0", lambda lib, L: lib.mpf_src_flow(ONE, ONE, 0, S, H, W, 0.0, ONE, None), "mpf_src_flow: P must be 1 or 2 (got 0)"),
    ("flow-S5000", lambda lib, L: lib.mpf_src_flow(ONE, ONE, 2, 5000, H, W, 0.0, ONE, None), "mpf_src_flow: bad shape S=5000 H=8 W=8"),
    ("flow-null-before-P", lambda lib, L: lib.mpf_src_flow(None, ONE, 3, S, H, W, 0.0, ONE, None), "mpf_src_flow: null pointer"),
    # ---- Stage B, several views ---------------------------------------------------------------------------------------------------------------------------
    ("views-null", lambda lib, L: wcv(lib, L, rgba=None), WCV + "null pointer"),
    ("views-n0", lambda lib, L: wcv(lib, L, n=0), WCV + "n_views must be 1..16 (got 0)"),
    ("views-n17", lambda lib, L: wcv(lib, L, n=17), WCV + "n_views must be 1..16 (got 17)"),
    ("views-planar", lambda lib, L: wcv(lib, L, inter=0), WCV + "the stack must be interleaved [S,H,W,4] (1, or 2 = tail-padded)"),
    ("views-S5000", lambda lib, L: wcv(lib, L, S=5000), WCV + "bad shape S=5000 H=8 W=8"),
    ("views-HW", lambda lib, L: wcv(lib, L, H=16384, W=8192), WCV + "H*W too large for 32-bit byte offsets"),
    ("views-misaligned-stack", lambda lib, L: wcv(lib, L, rgba=ODD), WCV + "the stack must be 16-byte aligned"),
    ("views-no-rgb", lambda lib, L: wcv(lib, L, vs=[dict(d_rgb=None)]), WCV + "view 0: null params / rgb"),
    ("views-no-params", lambda lib, L: wcv(lib, L, vs=[{}, dict(d_params=None)]), WCV + "view 1: null params / rgb"),
    ("views-mixed", lambda lib, L: wcv(lib, L, vs=[MASKED, {}]), WCV + "all views of a call take a mask, or none does"),
    ("views-mixed-the-other-way", lambda lib, L: wcv(lib, L, vs=[{}, MASKED]), WCV + "all views of a call take a mask, or none does"),
    ("views-quads-without-objmask", lambda lib, L: wcv(lib, L, vs=[dict(d_mask_quads=A(9))]), WCV + "view 0: mask quads and objmask output go together"),
    ("views-objmask-without-quads", lambda lib, L: wcv(lib, L, vs=[{}, dict(d_objmask=A(10))]), WCV + "view 1: mask quads and objmask output go together"),
    ("views-misaligned-quads", lambda lib, L: wcv(lib, L, vs=[MASKED, dict(d_mask_quads=260, d_objmask=A(11))]), WCV + "view 1: mask quads must be 16-byte aligned"),
    ("views-support-entry-n0", lambda lib, L: wcv(lib, L, "mpf_warp_composite_views_support", n=0, cells=[A(12)]), WCV + "n_views must be 1..16 (got 0)"),
    ("views-support-entry-mixed", lambda lib, L: wcv(lib, L, "mpf_warp_composite_views_support", vs=[MASKED, {}], cells=[A(12), A(12)]),
     WCV + "all views of a call take a mask, or none does"),
    ("views-support-entry-no-rgb", lambda lib, L: wcv(lib, L, "mpf_warp_composite_views_support", vs=[dict(d_rgb=None)]), WCV + "view 0: null params / rgb"),
    # two faults
    ("views-null-before-n", lambda lib, L: wcv(lib, L, rgba=None, n=0), WCV + "null pointer"),
    ("views-n-before-layout", lambda lib, L: wcv(lib, L, n=0, inter=0), WCV + "n_views must be 1..16 (got 0)"),
    ("views-stack-before-views", lambda lib, L: wcv(lib, L, rgba=ODD, vs=[dict(d_rgb=None)]), WCV + "the stack must be 16-byte aligned"),
    ("views-rgb-before-mixed", lambda lib, L: wcv(lib, L, vs=[MASKED, dict(d_rgb=None)]), WCV + "view 1: null params / rgb"),
    ("views-earlier-view-first", lambda lib, L: wcv(lib, L, vs=[dict(d_mask_quads=A(9)), dict(d_rgb=None)]), WCV + "view 0: mask quads and objmask output go together"),
    # ---- the pair launch ----------------------------------------------------------------------------------------------------------------------------------
    ("pair-P3", lambda lib, L: pair(lib, L, P=3, flows=A(3)), P_PAIR),
    ("pair-flows-with-P0", lambda lib, L: pair(lib, L, flows=A(3)), P_PAIR),
    ("pair-P2-without-flows", lambda lib, L: pair(lib, L, MERGE, P=2), P_PAIR),
    ("pair-quads-without-mask", lambda lib, L: pair(lib, L, quads=A(4)), PAIR + "quads need d_obj_mask_next"),
    ("pair-misaligned-quads", lambda lib, L: pair(lib, L, MERGE, obj_mask=A(5), quads=ODD), PAIR + "quads must be 16-byte aligned"),
    ("pair-misaligned-complement-quads", lambda lib, L: pair(lib, L, obj_mask=A(5), quads_c=ODD), PAIR + "quads must be 16-byte aligned"),
    ("pair-support-without-quads", lambda lib, L: pair(lib, L, MERGE_SUP, sup=A(6)), PAIR + "a support map needs its quads"),
    ("pair-complement-support-without-quads", lambda lib, L: pair(lib, L, MERGE_SUP, obj_mask=A(5), quads=A(4), sup=A(6), sup_c=A(7)), PAIR + "a support map needs its quads"),
    ("pair-S5000", lambda lib, L: pair(lib, L, S=5000), PAIR + "bad shape S=5000 H=8 W=8"),
    ("pair-same-stack", lambda lib, L: pair(lib, L, out=A(1)), PAIR + "the stack being rendered and the stack being written must be different buffers"),
    ("pair-null", lambda lib, L: pair(lib, L, mpi=None), PAIR + "null pointer"),
    ("pair-null-out", lambda lib, L: pair(lib, L, MERGE_SUP, out=None), PAIR + "null pointer"),
    ("pair-n0", lambda lib, L: pair(lib, L, n=0), PAIR + "n_views must be 1..16 (got 0)"),
    ("pair-n17", lambda lib, L: pair(lib, L, MERGE, n=17), PAIR + "n_views must be 1..16 (got 17)"),
    ("pair-HW", lambda lib, L: pair(lib, L, S=1, H=16384, W=8192), PAIR + "H*W too large for 32-bit byte offsets"),
    ("pair-4GiB", lambda lib, L: pair(lib, L, S=4000, H=1024, W=1024), GIB),
    ("pair-4GiB-merge-entry", lambda lib, L: pair(lib, L, MERGE_SUP, S=4000, H=1024, W=1024), GIB),
    ("pair-misaligned-stack", lambda lib, L: pair(lib, L, rgba=ODD), PAIR + "the stacks must be 16-byte aligned"),
    ("pair-misaligned-out", lambda lib, L: pair(lib, L, out=ODD), PAIR + "the stacks must be 16-byte aligned"),
    ("pair-view-no-rgb", lambda lib, L: pair(lib, L, vs=[dict(d_rgb=None)]), PAIR + "view 0: null params / rgb"),
    ("pair-mixed", lambda lib, L: pair(lib, L, MERGE, vs=[MASKED, {}]), PAIR + "all views of a call take a mask, or none does"),
    ("pair-view-quads-without-objmask", lambda lib, L: pair(lib, L, vs=[{}, dict(d_objmask=A(10))]), PAIR + "view 1: mask quads and objmask output go together"),
    ("pair-view-misaligned-quads", lambda lib, L: pair(lib, L, MERGE_SUP, vs=[dict(d_mask_quads=260, d_objmask=A(10))]), PAIR + "view 0: mask quads must be 16-byte aligned"),
    ("pair-view-tests-written-map", lambda lib, L: pair(lib, L, MERGE_SUP, vs=[MASKED, MASKED], cells=[A(12), A(6)], obj_mask=A(5), quads=A(4), sup=A(6)),
     PAIR + "view 1 tests a support map this launch writes"),
    ("pair-view-tests-written-complement-map", lambda lib, L: pair(lib, L, MERGE_SUP, vs=[MASKED], cells=[A(7)], obj_mask=A(5), quads=A(4), quads_c=A(13), sup=A(6), sup_c=A(7)),
     PAIR + "view 0 tests a support map this launch writes"),
    # two faults
    ("pair-null-before-same-stack", lambda lib, L: pair(lib, L, img=None, out=A(1)), PAIR + "null pointer"),
    ("pair-same-stack-before-n", lambda lib, L: pair(lib, L, out=A(1), n=0), PAIR + "the stack being rendered and the stack being written must be different buffers"),
    ("pair-n-before-shape", lambda lib, L: pair(lib, L, n=17, S=0), PAIR + "n_views must be 1..16 (got 17)"),
    ("pair-shape-before-P", lambda lib, L: pair(lib, L, S=5000, P=3), PAIR + "bad shape S=5000 H=8 W=8"),
    ("pair-4GiB-before-alignment", lambda lib, L: pair(lib, L, rgba=ODD, S=4000, H=1024, W=1024), GIB),
    ("pair-alignment-before-P", lambda lib, L: pair(lib, L, rgba=ODD, P=3), PAIR + "the stacks must be 16-byte aligned"),
    ("pair-P-before-quads", lambda lib, L: pair(lib, L, P=3, quads=A(4)), P_PAIR),
    ("pair-mask-before-alignment", lambda lib, L: pair(lib, L, quads=ODD), PAIR + "quads need d_obj_mask_next"),
    ("pair-alignment-before-support", lambda lib, L: pair(lib, L, MERGE_SUP, obj_mask=A(5), quads_c=ODD, sup=A(6)), PAIR + "quads must be 16-byte aligned"),
    ("pair-support-before-written-map", lambda lib, L: pair(lib, L, MERGE_SUP, cells=[A(6)], sup=A(6)), PAIR + "a support map needs its quads"),
    ("pair-written-map-before-views", lambda lib, L: pair(lib, L, MERGE_SUP, vs=[dict(d_rgb=None)], cells=[A(6)], obj_mask=A(5), quads=A(4), sup=A(6)),
     PAIR + "view 0 tests a support map this launch writes"),
    ("pair-stage-ac-before-views", lambda lib, L: pair(lib, L, vs=[dict(d_rgb=None)], flows=A(3)), P_PAIR),
    # ---- the merge folded into the pair launch ------------------------------------------------------------------------------------------------------------
    ("merge-null-member", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_mask_dyn=None)), MP + "merge_prev has a null pointer"),
    ("merge-null-output", lambda lib, L: pair(lib, L, MERGE_SUP, mg=dict(d_fill_mask=None)), MP + "merge_prev has a null pointer"),
    ("merge-renders-its-own-input", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_frame_dyn=A(8))), MP + "the merged pair's views must not be the views this launch renders"),
    ("merge-renders-its-own-mask", lambda lib, L: pair(lib, L, MERGE, vs=[MASKED], mg=dict(d_mask=A(10))), MP + "the merged pair's views must not be the views this launch renders"),
    ("merge-stride5", lambda lib, L: pair(lib, L, MERGE, mg=dict(obj_mask_stride=5)), MP + "obj_mask_stride must be 0..4"),
    ("merge-flows-off-plane", lambda lib, L: pair(lib, L, MERGE, P=2, flows=A(3), mg=dict(d_flow=A(3) + 4 * N)), FLOWS),
    ("merge-dyn-flows-off-plane", lambda lib, L: pair(lib, L, MERGE_SUP, P=2, flows=A(3), mg=dict(d_flow=A(3), d_flow_dyn=A(3) + 12 * N)), FLOWS),
    ("merge-flows-on-plane-but-P1", lambda lib, L: pair(lib, L, MERGE, P=1, flows=A(3), mg=dict(d_flow=A(3))), FLOWS),
    ("merge-mask-is-written-quads", lambda lib, L: pair(lib, L, MERGE, obj_mask=A(5), quads=A(4), mg=dict(d_obj_mask=A(4))), OBJ),
    ("merge-mask-is-written-stack", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_obj_mask=A(2) + 4096 - 4)), OBJ),
    ("merge-flow-mix-on-next-stack", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_flow_mix=A(2))), MP + "merge_prev's flow_mix overlaps a buffer this launch reads or writes"),
    ("merge-frame-mix-on-read-stack", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_frame_mix=A(1) + 4000)), MP + "merge_prev's frame_mix overlaps a buffer this launch reads or writes"),
    ("merge-fill-mask-on-view", lambda lib, L: pair(lib, L, MERGE_SUP, mg=dict(d_fill_mask=A(8) + 700)), MP + "merge_prev's fill_mask overlaps a buffer this launch reads or writes"),
    ("merge-outputs-on-each-other", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_frame_mix=A(27) + 8)), MP + "merge_prev's flow_mix overlaps a buffer this launch reads or writes"),
    ("merge-output-on-its-input", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_fill_mask=A(22) + 255)), MP + "merge_prev's fill_mask overlaps a buffer this launch reads or writes"),
    # two faults: the merge is judged first, and in its own order
    ("merge-before-null", lambda lib, L: pair(lib, L, MERGE, mpi=None, mg=dict(obj_mask_stride=5)), MP + "obj_mask_stride must be 0..4"),
    ("merge-before-same-stack", lambda lib, L: pair(lib, L, MERGE_SUP, out=A(1), mg=dict(d_frame=None)), MP + "merge_prev has a null pointer"),
    ("merge-null-before-stride", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_flow=None, obj_mask_stride=-1)), MP + "merge_prev has a null pointer"),
    ("merge-views-before-stride", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_frame=A(8), obj_mask_stride=5)), MP + "the merged pair's views must not be the views this launch renders"),
    ("merge-stride-before-flows", lambda lib, L: pair(lib, L, MERGE, P=2, flows=A(3), mg=dict(d_flow=A(3) + 4, obj_mask_stride=7)), MP + "obj_mask_stride must be 0..4"),
    ("merge-flows-before-mask", lambda lib, L: pair(lib, L, MERGE, P=2, flows=A(3), mg=dict(d_flow=A(3) + 4, d_obj_mask=A(2))), FLOWS),
    ("merge-mask-before-outputs", lambda lib, L: pair(lib, L, MERGE, mg=dict(d_obj_mask=A(2), d_flow_mix=A(2))), OBJ),
    ("merge-null-views-still-judged", lambda lib, L: lib.mpf_warp_views_blend_next_merge_prev(
        ctypes.c_void_p(A(1)), None, 1, ONE, ONE, ONE, 0, 0.0, ctypes.c_void_p(A(2)), None, None, None, None, None, None, S, H, W, ctypes.byref(merge(L, obj_mask_stride=5)), None),
     MP + "obj_mask_stride must be 0..4"),
    ("merge-passes-then-null-views", lambda lib, L: lib.mpf_warp_views_blend_next_merge_prev(
        ctypes.c_void_p(A(1)), None, 1, ONE, ONE, ONE, 0, 0.0, ctypes.c_void_p(A(2)), None, None, None, None, None, None, S, H, W, ctypes.byref(merge(L)), None),
     PAIR + "null pointer"),
]


def test_the_table_names_each_row_once():
    ids = [r[0] for r in ROWS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("call,want", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_bad_arguments_are_refused_with_this_message(built, call, want):
    lib = built.load()
    rc = call(lib, built)
    assert (rc, lib.mpf_last_error()) == (10001, want.encode())
