"""CPU: host logic of block.py that needs no device -- the light-shape rules of the many-lights entries and the signature that
ties a march call to its prepass (round 6)."""
import pytest
import torch


def test_light_shapes_one_light_and_many_lights_forms():
    from geomconsistentfr_amd import block as R
    from geomconsistentfr_amd._lib import GcfrError
    B = 4
    l3, a2, L, multi = R._light_shapes(B, torch.zeros(B, 3), torch.zeros(B))
    assert (tuple(l3.shape), tuple(a2.shape), L, multi) == ((B, 1, 3), (B, 1), 1, False)
    l3, a2, L, multi = R._light_shapes(B, torch.zeros(B, 3, 1, 1), torch.zeros(B, 1, 1))          # the scripts' target_lighting (S1:588)
    assert (tuple(l3.shape), L, multi) == ((B, 1, 3), 1, False)
    l3, a2, L, multi = R._light_shapes(B, torch.zeros(B, 11, 3), torch.zeros(B, 11))
    assert (tuple(l3.shape), tuple(a2.shape), L, multi) == ((B, 11, 3), (B, 11), 11, True)
    l3, a2, L, multi = R._light_shapes(B, torch.zeros(B, 1, 3), torch.zeros(B, 1))                # L = 1 WITH a light axis
    assert (L, multi) == (1, True)
    sl = torch.zeros(B, 1, 1, 4)
    l3, a2, L, multi = R._light_shapes(B, sl[:, 0, 0, 1:4], sl[:, 0, 0, 0])                        # the training form's slices (T8:357, 367)
    assert l3.data_ptr() == sl[:, 0, 0, 1:4].data_ptr() and not multi                             # a view: no copy
    with pytest.raises(GcfrError):
        R._light_shapes(B, torch.zeros(B, 11, 3), torch.zeros(B, 10))
    with pytest.raises(GcfrError):
        R._light_shapes(B, torch.zeros(B, 4), torch.zeros(B))


def test_source_signature_sees_other_tensors_views_and_in_place_writes():
    from geomconsistentfr_amd import block as R
    d, m, l = torch.rand(2, 1, 8, 8), torch.ones(2, 8, 8), torch.rand(2, 3)
    s0 = R.source_signature(d, m, l)
    assert s0 == R.source_signature(d, m, l)
    assert s0 == R.source_signature(d.detach(), m, l.detach())                # autograd's detached aliases: same storage, same counter
    assert s0 != R.source_signature(d.clone(), m, l)                          # another tensor with the same values
    assert s0 != R.source_signature(d, m, l[:, :3].flip(0))                   # another view / layout
    assert s0 != R.source_signature(d.reshape(2, 8, 8), m, l)                 # the same storage under another shape
    d.add_(1.0)                                                               # written in place: the version counter moves ...
    assert s0 != R.source_signature(d, m, l)
    v = d.reshape(2, 8, 8)
    s1 = R.source_signature(v, m, l)
    d.mul_(2.0)                                                               # ... for every view of the tensor
    assert s1 != R.source_signature(v, m, l)


def test_normals_stage_rule_and_result_shapes():
    from geomconsistentfr_amd import block as R
    assert R.normals_stage_for(1) == "fused" and R.normals_stage_for(11) == "fused" and R.normals_stage_for(18) == "kernel"
    B, L, H, W = 2, 3, 4, 5
    z = lambda *s: torch.zeros(*s)
    r = R._result_dict(B, H, W, True, z(B, L), z(B, L, H, W), z(B, L, H, W), z(B, L, H, W), z(B, L, 3, H, W), z(B, L, 3), z(B, L, H, W),
                       normals=z(B, 3, H, W))
    assert tuple(r["rendered_images"].shape) == (B, L, 3, H, W) and tuple(r["unit_light_direction"].shape) == (B, L, 3, 1, 1)
    assert tuple(r["ambient_light"].shape) == (B, L, H, W) and tuple(r["ambient_values"].shape) == (B, L, 1, 1)
    r = R._result_dict(B, H, W, False, z(B, 1), z(B, 1, H, W), z(B, 1, H, W), z(B, 1, H, W), z(B, 1, 3, H, W), z(B, 1, 3), z(B, 1, H, W))
    assert tuple(r["rendered_images"].shape) == (B, 3, H, W) and tuple(r["unit_light_direction"].shape) == (B, 3, 1, 1)   # T8:524
    assert tuple(r["ambient_light"].shape) == (B, H, W) and tuple(r["ambient_values"].shape) == (B, 1, 1)


def test_camera_scalars_cache_follows_the_tensor_object_and_its_version():
    """camera_scalars caches per tensor OBJECT (host tensors too since round 6: the read is 10 us of tensor arithmetic per call):
    an in-place write invalidates the entry, a dead tensor's entry is dropped, per-image matrices give None."""
    import gc
    from geomconsistentfr_amd import block as R
    K = torch.zeros(1, 3, 3, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = 1570.0
    K[:, 2, 2] = 1.0
    K[:, 0, 2], K[:, 1, 2] = 128.0, 120.0
    n0 = len(R._CAMERA_CACHE)
    assert R.camera_scalars(K) == (1570.0, 1570.0, 128.0, 120.0) and len(R._CAMERA_CACHE) == n0 + 1
    assert R.camera_scalars(K) == (1570.0, 1570.0, 128.0, 120.0)                     # served from the cache
    K[:, 0, 0] = 700.0                                                                # in place: the version counter moves
    assert R.camera_scalars(K)[0] == 700.0
    two = torch.cat([K, K]).clone()
    assert R.camera_scalars(two) == (700.0, 1570.0, 128.0, 120.0)                     # B equal matrices
    two[1, 0, 0] = 900.0
    assert R.camera_scalars(two) is None                                              # per-image matrices: the three-stage path
    del K, two
    gc.collect()
    assert len(R._CAMERA_CACHE) == n0


def test_source_signature_and_camera_scalars_take_inference_tensors():
    """Tensors made under torch.inference_mode() have no version counter (reading `_version` raises): the signature records
    None in its place -- a weaker check, stated in its docstring -- and camera_scalars reads such a matrix every time and never
    caches it, so an in-place write is still seen.  A normal tensor handed over inside inference mode keeps its counter."""
    from geomconsistentfr_amd import block as R
    n0 = len(R._CAMERA_CACHE)
    d_normal = torch.rand(2, 1, 8, 8)
    with torch.inference_mode():
        d, m, l = torch.rand(2, 1, 8, 8), torch.ones(2, 8, 8), torch.rand(2, 3)
        s0 = R.source_signature(d, m, l)
        assert s0 == R.source_signature(d, m, l) and [e[1] for e in s0] == [None] * 3
        assert s0 != R.source_signature(d.clone(), m, l)
        assert s0 != R.source_signature(d.reshape(2, 8, 8), m, l)
        assert R.source_signature(d_normal, m, l)[0][1] == d_normal._version
        K = torch.zeros(1, 3, 3, dtype=torch.float64)
        K[:, 0, 0] = K[:, 1, 1] = 1570.0
        K[:, 2, 2] = 1.0
        K[:, 0, 2], K[:, 1, 2] = 128.0, 120.0
        assert K.is_inference()
        assert R.camera_scalars(K) == (1570.0, 1570.0, 128.0, 120.0)
        assert len(R._CAMERA_CACHE) == n0                                            # not cached
        K[:, 0, 0] = 700.0
        assert R.camera_scalars(K) == (700.0, 1570.0, 128.0, 120.0)
        two = torch.cat([K, K])
        two[1, 0, 0] = 900.0
        assert R.camera_scalars(two) is None
    assert R.camera_scalars(K)[0] == 700.0 and len(R._CAMERA_CACHE) == n0             # outside inference mode too


_FORWARD_ENTRIES = ("gcfr_render_fwd", "gcfr_render_from_depth_fwd", "gcfr_normals_fwd")


def _prototype_names(entry):
    """the parameter names of `entry`'s prototype in include/gcfr.h, in order: the text between the entry's name and the
    closing `);`, split on commas; the last identifier of each piece"""
    import os
    import re
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "gcfr.h")) as f:
        text = f.read()
    m = re.search(r"\bint\s+%s\s*\((.*?)\);" % entry, text, re.S)
    assert m, entry
    return [re.findall(r"[A-Za-z_]\w*", piece)[-1] for piece in m.group(1).split(",")]


def _fake_arguments(entry):
    """one distinct value per parameter of `entry`, of the kind its ctypes argtype takes: a fake address for a pointer, an int
    for an integer, a float for a floating-point parameter"""
    import ctypes
    from geomconsistentfr_amd import _lib
    names, argtypes = _prototype_names(entry), _lib._SIGNATURES[entry][1]
    assert len(names) == len(argtypes)
    kw = {}
    for i, (n, t) in enumerate(zip(names, argtypes)):
        kw[n] = 0.5 + i if t in (ctypes.c_float, ctypes.c_double) else (0x10000 + 0x100 * i if t is ctypes.c_void_p else 3 + i)
    return names, argtypes, kw


@pytest.mark.parametrize("entry", _FORWARD_ENTRIES)
def test_forward_argument_builders_follow_the_header_prototypes(entry):
    """block.py's three builders are the only places that spell the forward entries' argument orders; ctypes checks a type per
    position only and the lists hold runs of up to nine `void *`.  Each builder is held to its prototype in include/gcfr.h:
    the value passed under the header's i-th parameter name sits at position i, in a form its argtype accepts."""
    import ctypes
    from geomconsistentfr_amd import _lib
    from geomconsistentfr_amd import block as R
    builder = getattr(R, "_" + entry[len("gcfr_"):] + "_args")
    names, argtypes, kw = _fake_arguments(entry)
    assert len(set(kw.values())) == len(names)
    args = builder(**kw)
    assert isinstance(args, tuple) and len(args) == len(_lib._SIGNATURES[entry][1])
    for i, (n, t) in enumerate(zip(names, argtypes)):
        assert args[i] is kw[n] or args[i] == kw[n], (i, n)
        t.from_param(args[i])
        if t in (ctypes.c_float, ctypes.c_double):
            assert type(args[i]) is float, (i, n)
    missing = dict(kw)
    del missing[names[len(names) // 2]]
    with pytest.raises(TypeError):
        builder(**missing)
    with pytest.raises(TypeError):
        builder(**kw, no_such_parameter=1)
    with pytest.raises(TypeError):
        builder(*kw.values())                                                   # by keyword only


def _bound_forward(camera, stage, prepass=False):
    """`block._Forward.bind()` on host tensors (it only takes their addresses) -> the header's names, the bound launches and
    the address each pointer parameter has to carry"""
    from geomconsistentfr_amd import RenderParams
    from geomconsistentfr_amd import block as R
    B, L, H, W = 2, 3, 4, 6
    t = {n: torch.zeros(8) for n in ("light", "depth", "mask_u8", "normals", "albedo", "ambient", "ws", "unit_light_direction", "light_pt",
                                     "minimum_distance", "argmin", "shadow_mask_weights", "full_shading", "final_shading",
                                     "rendered_images", "surface_normals")}
    fwd = R._Forward(RenderParams(n_samples=24, dt=0.03, bonus_box=(-3.0, 2.0, -1.0, 2.0)), B, L, H, W, "cpu", camera, stage)
    out = {n: t[n] for n in (("unit_light_direction", "light_pt") if prepass else list(t)[7:15 if camera is None else 16])}
    given = [None if prepass or camera is not None else t["normals"]] + [None if prepass else t[n] for n in ("albedo", "ambient")]
    bound = fwd.bind(t["light"], t["depth"], t["mask_u8"], B, *given, out, t["ws"], 4096)
    expect = dict(light_raw="light", depth="depth", mask_u8="mask_u8", albedo="albedo", ambient="ambient", workspace="ws",
                  unit_out="unit_light_direction", light_pt_out="light_pt", min_dist="minimum_distance", argmin="argmin",
                  shadow_w="shadow_mask_weights", full="full_shading", final_shading="final_shading", rendered="rendered_images")
    return bound, {k: t[v].data_ptr() for k, v in expect.items()}, t, fwd


def test_prepass_form_leaves_exactly_the_operands_it_does_not_have_null():
    """The prepass is the gcfr_render_fwd list at phase 1 without albedo, ambient, normals and march outputs: None at exactly
    those positions, real values at the light outputs and the workspace."""
    names = _prototype_names("gcfr_render_fwd")
    (normals_launch, args), addr, _, _ = _bound_forward(None, "fused", prepass=True)
    absent = ["normals", "albedo", "ambient", "min_dist", "argmin", "shadow_w", "full", "final_shading", "rendered"]
    assert normals_launch is None and [n for n, a in zip(names, args) if a is None] == absent
    for n in ("light_raw", "depth", "mask_u8", "unit_out", "light_pt_out", "workspace"):
        assert args[names.index(n)] == addr[n], n
    assert args[names.index("workspace_bytes")] == 4096 and args[names.index("N")] == 24


@pytest.mark.parametrize("form", ["given", "kernel", "fused"])
def test_bound_launches_carry_each_tensor_under_its_header_name(form):
    """The three forms of the forward as `render_fwd` / `RenderFwdPlan` bind them: every pointer parameter of the header
    carries the address of the tensor of that role, and the normals stage's output is what the march reads ("kernel") or
    writes ("fused")."""
    camera = None if form == "given" else (1570.0, 1571.0, 3.0, 2.0, 1610.0)
    (normals_launch, args), addr, t, fwd = _bound_forward(camera, form)
    names = _prototype_names("gcfr_render_from_depth_fwd" if form == "fused" else "gcfr_render_fwd")
    assert len(args) == len(names)
    for n, a in addr.items():
        assert args[names.index(n)] == a, n
    got = dict(zip(names, args))
    assert (got["B"], got["L"], got["H"], got["W"], got["N"], got["mask_batch"]) == (2, 3, 4, 6, 24, 2)
    assert got["stream"] is fwd.stream and got["opt"] is fwd.opt               # (the two cells a call fills in)
    if form == "given":
        assert normals_launch is None and got["normals"] == t["normals"].data_ptr()
        return
    nrm = t["surface_normals"].data_ptr()
    assert got["normals_out" if form == "fused" else "normals"] == nrm
    cam = dict(fx=1570.0, fy=1571.0, cx=3.0, cy=2.0, z_offset=1610.0, negate_y=1)
    if form == "fused":
        assert normals_launch is None and {k: got[k] for k in cam} == cam
    else:
        g = dict(zip(_prototype_names("gcfr_normals_fwd"), normals_launch))
        assert {k: g[k] for k in cam} == cam and (g["depth"], g["B"], g["H"], g["W"], g["normals"]) == (addr["depth"], 2, 4, 6, nrm)
        assert g["stream"] is fwd.stream
