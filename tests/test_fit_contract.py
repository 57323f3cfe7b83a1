"""CPU-only: the argument contract of the fit entry points of the C-ABI (la3d_fit_instances, _rle, _poly, _rle_filtered,
_poly_filtered, _ex).  Every call here is either rejected before the library touches HIP - return code and la3d_last_error
text are checked - or has B = 0 and succeeds without doing anything.  The pointers are NOT device memory (any non-null,
16-aligned value serves: nothing may dereference them), so the module skips itself where a GPU is visible: a call that got
past the checks there would launch a kernel on them."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: CPU-only contract test")

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
PTR = 0x10000      # stands for any device buffer (16-aligned, never dereferenced)
ODD = PTR + 4      # not 8-aligned

LEGACY = ("la3d_fit_instances", "la3d_fit_instances_rle", "la3d_fit_instances_poly", "la3d_fit_instances_rle_filtered",
          "la3d_fit_instances_poly_filtered")


def _base(B=1, H=8, W=32):
    return dict(depth=PTR, depth_plane_stride=0, image_index=None, mask=PTR, rle_counts=PTR, rle_offsets=PTR, poly_xy=PTR,
                ring_offsets=PTR, inst_rings=PTR, K=PTR, k_stride=0, ground=None, sample_idx=None, B=B, H=H, W=W,
                boundary=10, min_area=100, max_edge=10, out=PTR, status=PTR, aux=None, stats=None, workspace=PTR, stream=None)


def _call_legacy(lib, name, kw):
    """One legacy entry with the fields of `kw` it takes, in its own argument order."""
    head = [kw["depth"], kw["depth_plane_stride"], kw["image_index"]]
    cam = [kw["K"], kw["k_stride"], kw["ground"], kw["sample_idx"], kw["B"], kw["H"], kw["W"]]
    masks = {"la3d_fit_instances": [kw["mask"]], "la3d_fit_instances_rle": [kw["rle_counts"], kw["rle_offsets"]],
             "la3d_fit_instances_poly": [kw["poly_xy"], kw["ring_offsets"], kw["inst_rings"]]}
    kind = name.replace("_filtered", "")
    if name.endswith("_filtered"):
        args = head + masks[kind] + cam + [kw["boundary"], kw["min_area"], kw["max_edge"], kw["out"], kw["status"], kw["aux"],
                                           kw["stats"], kw["workspace"], kw["stream"]]
    else:
        args = head + masks[kind] + cam + [kw["out"], kw["status"], kw["aux"], kw["workspace"], kw["stream"]]
    return getattr(lib, name)(*args)


def _call_ex(lib, fields, struct_size=None):
    from labelany3d_amd._lib import FitArgs

    a = FitArgs()
    a.struct_size = C.sizeof(FitArgs) if struct_size is None else struct_size
    a.filter_boundary = -1
    for k, v in fields.items():
        setattr(a, k, v)
    return lib.la3d_fit_instances_ex(C.byref(a))


def _ex_fields(kind="mask", B=1, H=8, W=32, **over):
    f = dict(B=B, H=H, W=W, depth=PTR, K=PTR, out=PTR, status=PTR, workspace=PTR)
    f.update({"mask": dict(mask=PTR), "rle": dict(rle_counts=PTR, rle_offsets=PTR),
              "poly": dict(poly_xy=PTR, ring_offsets=PTR, inst_rings=PTR)}[kind])
    f.update(over)
    return f


def _only(name, kw):
    """`kw` with the mask pointers of the other kinds cleared (the legacy entries take one kind each)."""
    kind = name.replace("la3d_fit_instances", "").replace("_filtered", "") or "_u8"
    keep = {"_u8": ("mask",), "_rle": ("rle_counts", "rle_offsets"), "_poly": ("poly_xy", "ring_offsets", "inst_rings")}[kind]
    for k in ("mask", "rle_counts", "rle_offsets", "poly_xy", "ring_offsets", "inst_rings"):
        if k not in keep:
            kw[k] = None
    return kw


# (fields changed from _base, expected rc, expected error text after "<entry>: ") for every legacy entry
COMMON = [
    (dict(depth=None), ERR_ARG, "bad argument"),
    (dict(K=None), ERR_ARG, "bad argument"),
    (dict(out=None), ERR_ARG, "bad argument"),
    (dict(status=None), ERR_ARG, "bad argument"),
    (dict(B=-1), ERR_ARG, "bad argument"),
    (dict(H=0), ERR_ARG, "bad argument"),
    (dict(W=-32), ERR_ARG, "bad argument"),
    (dict(depth_plane_stride=-1), ERR_ARG, "bad argument"),
    (dict(k_stride=8), ERR_ARG, "bad argument"),
    (dict(k_stride=-9), ERR_ARG, "bad argument"),
    (dict(H=16385, W=16384), ERR_ARG, "bad argument"),                  # H*W > 2^28
    (dict(H=16385, W=16384, B=0), ERR_ARG, "bad argument"),             # (checked before B == 0)
    (dict(workspace=None), ERR_ARG, "workspace of la3d_workspace_bytes() bytes (8-aligned) required"),
    (dict(workspace=ODD), ERR_ARG, "workspace of la3d_workspace_bytes() bytes (8-aligned) required"),
]
MASK_NULL = {"la3d_fit_instances": dict(mask=None), "la3d_fit_instances_rle": dict(rle_counts=None),
             "la3d_fit_instances_rle_filtered": dict(rle_counts=None), "la3d_fit_instances_poly": dict(poly_xy=None),
             "la3d_fit_instances_poly_filtered": dict(poly_xy=None)}
LDS_TOO_SMALL = dict(H=1024, W=2048)   # the bit image of a run-length / polygon frame does not fit in LDS


def _legacy_cases():
    out = []
    for name in LEGACY:
        for i, (over, rc, msg) in enumerate(COMMON):
            out.append((name, over, rc, msg, f"common{i}"))
        out.append((name, MASK_NULL[name], ERR_ARG, "bad argument", "mask_null"))
        # (a polygon call of zero instances needs no vertices; the others still need their mask pointer)
        b0_ok = "poly" in name
        out.append((name, dict(MASK_NULL[name], B=0), OK if b0_ok else ERR_ARG, None if b0_ok else "bad argument", "mask_null_B0"))
        out.append((name, dict(B=0), OK, None, "B0"))
        out.append((name, dict(B=0, workspace=None), OK, None, "B0_no_workspace"))
        if name != "la3d_fit_instances":
            out.append((name, LDS_TOO_SMALL, ERR_UNSUPPORTED,
                        "run-length / polygon masks need the bit image in LDS (H*W <= 1048576)", "lds"))
    out += [
        ("la3d_fit_instances_rle", dict(rle_offsets=None), ERR_ARG, "bad argument", "offsets_null"),
        ("la3d_fit_instances_rle_filtered", dict(rle_offsets=None), ERR_ARG, "bad argument", "offsets_null"),
        ("la3d_fit_instances_poly", dict(ring_offsets=None), ERR_ARG, "bad argument", "rings_null"),
        ("la3d_fit_instances_poly", dict(inst_rings=None), ERR_ARG, "bad argument", "inst_null"),
        ("la3d_fit_instances_poly", dict(inst_rings=None, B=0), ERR_ARG, "bad argument", "inst_null_B0"),
        ("la3d_fit_instances_poly_filtered", dict(ring_offsets=None), ERR_ARG, "bad argument", "rings_null"),
        # the *_filtered entries always run the filter: it wants boundary >= 0 (max_edge <= 0 is accepted: it drops everything)
        ("la3d_fit_instances_rle_filtered", dict(boundary=-1), ERR_ARG,
         "the fused filter needs run-length or polygon masks and boundary >= 0", "boundary"),
        ("la3d_fit_instances_poly_filtered", dict(boundary=-1), ERR_ARG,
         "the fused filter needs run-length or polygon masks and boundary >= 0", "boundary"),
        ("la3d_fit_instances_rle_filtered", dict(boundary=-1, B=0), OK, None, "boundary_B0"),
        ("la3d_fit_instances_poly_filtered", dict(boundary=-1, B=0), OK, None, "boundary_B0"),
        ("la3d_fit_instances_rle_filtered", dict(boundary=-1, workspace=None), ERR_ARG,
         "workspace of la3d_workspace_bytes() bytes (8-aligned) required", "workspace_first"),
        ("la3d_fit_instances_poly_filtered", dict(boundary=-1) | LDS_TOO_SMALL, ERR_ARG,
         "the fused filter needs run-length or polygon masks and boundary >= 0", "filter_before_lds"),
    ]
    return out


@pytest.mark.parametrize("name,over,rc,msg,tag", _legacy_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_legacy_entry_contract(name, over, rc, msg, tag):
    from labelany3d_amd._lib import lib

    kw = _only(name, _base())
    kw.update(over)
    assert _call_legacy(lib, name, kw) == rc
    if msg is not None:
        assert lib.la3d_last_error().decode() == f"{name}: {msg}"


EX = "la3d_fit_instances_ex"
V1_SIZE = 200      # the block as first published: every field up to `stream` (offset of area_hint)
FILTER = dict(filter_boundary=10, filter_min_area=100, filter_max_edge=10)


def _ex_cases():
    out = []
    for kind in ("mask", "rle", "poly"):
        for i, (over, rc, msg) in enumerate(COMMON):
            out.append((kind, over, None, rc, msg, f"common{i}"))
        out.append((kind, dict(B=0), None, OK, None, "B0"))
        out.append((kind, dict(B=0, workspace=0), None, OK, None, "B0_no_workspace"))
        out.append((kind, dict(frame_width=-1), None, ERR_ARG,
                    "frame_width must be 0 or in (0, W], with run-length / polygon masks and W % 32 == 0", "frame_neg"))
        out.append((kind, dict(frame_width=33), None, ERR_ARG,
                    "frame_width must be 0 or in (0, W], with run-length / polygon masks and W % 32 == 0", "frame_wide"))
        out.append((kind, dict(frame_width=20, W=48), None, ERR_ARG,
                    "frame_width must be 0 or in (0, W], with run-length / polygon masks and W % 32 == 0", "frame_w32"))
        out.append((kind, dict(proj=PTR), None, ERR_ARG, "proj needs image_width / image_height > 0", "proj"))
        out.append((kind, dict(proj=PTR, image_width=640.0), None, ERR_ARG, "proj needs image_width / image_height > 0", "proj_h"))
        for field, bad in (("opt_engine", -1), ("opt_engine", 6), ("opt_launch_order", -1), ("opt_launch_order", 3),
                           ("opt_build", -1), ("opt_build", 3)):
            out.append((kind, {field: bad}, None, ERR_ARG, "bad opt_engine / opt_launch_order / opt_build", f"{field}{bad}"))
        out.append((kind, dict(opt_engine=1, B=-1), None, ERR_ARG, "bad argument", "opts_ok_then_dispatch"))
        out.append((kind, {}, 0, ERR_ARG, "bad struct_size", "size0"))
        out.append((kind, {}, 8, ERR_ARG, "bad struct_size", "size8"))
        out.append((kind, dict(B=0), V1_SIZE, OK, None, "v1_block_B0"))
        out.append((kind, dict(B=0), V1_SIZE - 1, ERR_ARG, "bad struct_size", "v1_short"))
    out += [
        ("mask", dict(frame_width=20), None, ERR_ARG,
         "frame_width must be 0 or in (0, W], with run-length / polygon masks and W % 32 == 0", "frame_u8"),
        ("mask", dict(FILTER), None, ERR_ARG, "the fused filter needs run-length or polygon masks and boundary >= 0", "filter_u8"),
        ("mask", dict(FILTER, B=0), None, OK, None, "filter_u8_B0"),
        ("rle", dict(FILTER, workspace=0), None, ERR_ARG, "workspace of la3d_workspace_bytes() bytes (8-aligned) required",
         "filter_workspace"),
        ("rle", dict(FILTER) | LDS_TOO_SMALL, None, ERR_UNSUPPORTED,
         "run-length / polygon masks need the bit image in LDS (H*W <= 1048576)", "filter_lds"),
        ("poly", dict(FILTER) | LDS_TOO_SMALL, None, ERR_UNSUPPORTED,
         "run-length / polygon masks need the bit image in LDS (H*W <= 1048576)", "filter_lds"),
        ("rle", LDS_TOO_SMALL, None, ERR_UNSUPPORTED, "run-length / polygon masks need the bit image in LDS (H*W <= 1048576)", "lds"),
        ("poly", LDS_TOO_SMALL, None, ERR_UNSUPPORTED, "run-length / polygon masks need the bit image in LDS (H*W <= 1048576)", "lds"),
        # the filter is on only when filter_boundary >= 0 AND filter_max_edge > 0: otherwise u8 masks pass the filter check
        ("mask", dict(filter_boundary=10, filter_max_edge=0, workspace=0), None, ERR_ARG,
         "workspace of la3d_workspace_bytes() bytes (8-aligned) required", "filter_off_edge"),
        ("mask", dict(filter_boundary=-1, filter_max_edge=10, workspace=0), None, ERR_ARG,
         "workspace of la3d_workspace_bytes() bytes (8-aligned) required", "filter_off_boundary"),
        ("rle", dict(rle_offsets=0), None, ERR_ARG, "bad argument", "offsets_null"),
        ("poly", dict(ring_offsets=0), None, ERR_ARG, "polygon masks need ring_offsets and inst_rings", "rings_null"),
        ("poly", dict(inst_rings=0, B=0), None, ERR_ARG, "polygon masks need ring_offsets and inst_rings", "inst_null_B0"),
        ("mask", dict(rle_counts=PTR, rle_offsets=PTR), None, ERR_ARG, "give exactly one of mask / rle_counts / poly_xy", "two_kinds"),
        ("rle", dict(poly_xy=PTR, ring_offsets=PTR, inst_rings=PTR), None, ERR_ARG, "give exactly one of mask / rle_counts / poly_xy",
         "two_kinds"),
        ("mask", dict(mask=0), None, ERR_ARG, "give exactly one of mask / rle_counts / poly_xy", "no_kind"),
        ("mask", dict(mask=0, B=0), None, ERR_ARG, "bad argument", "no_kind_B0"),
        ("mask", dict(rle_counts=PTR, rle_offsets=PTR, B=0), None, OK, None, "two_kinds_B0"),
        ("rle", dict(frame_width=20, workspace=0), None, ERR_ARG, "workspace of la3d_workspace_bytes() bytes (8-aligned) required",
         "frame_after_workspace"),
    ]
    return out


@pytest.mark.parametrize("kind,over,size,rc,msg,tag", _ex_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_ex_contract(kind, over, size, rc, msg, tag):
    from labelany3d_amd._lib import lib

    fields = _ex_fields(kind)
    fields.update(over)
    assert _call_ex(lib, fields, size) == rc
    if msg is not None:
        assert lib.la3d_last_error().decode() == f"{EX}: {msg}"


def test_ex_null_block():
    from labelany3d_amd._lib import FitArgs, lib

    assert FitArgs.area_hint.offset == V1_SIZE

    assert lib.la3d_fit_instances_ex(None) == ERR_ARG
    assert lib.la3d_last_error().decode() == f"{EX}: bad struct_size"
