"""Procedural textures on the CPU: the product's texture code compiled for the host
(tests/hostcheck/tex_check.cpp) against the fixtures the real reference produced
(tests/golden/textures/, tests/js/texture_reference.mjs), the three loaders' agreement on the scene-JSON
"texture" extension, the keyed texture permutations, the lowering of constant textures and the descriptor
validation.  The GPU side is tests/test_textures_gpu.py."""
import base64
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import texcheck_binding as tb
from blenderraytracer_amd import capi
from blenderraytracer_amd.rng import permutation, texture_permutation
from blenderraytracer_amd.scene import (PackedScene, World, default_scene, load_from_json, load_scene_json, scene_path,
                                        keyed_texture_permutation)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "js", "texture_host_tool.mjs")
NODE = shutil.which("node")
needs_node = pytest.mark.skipif(NODE is None, reason="node not installed")
SIN_LIMIT = 2.0 ** 19 * np.pi / 2


def run_tool(*args):
    out = subprocess.run([NODE, TOOL, *args], cwd=ROOT, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return json.loads(out.stdout)


# ---- fixtures are inside the exact range ---------------------------------------------------------------
def test_fixtures_stay_inside_the_exact_range():
    m = tb.manifest()
    assert sorted(m["cases"]) == sorted(tb.CASES)
    for r in [c["range"] for c in m["cases"].values()] + [m["kats_range"], tb.kats()["range"]]:
        assert r["max_sin_argument"] <= SIN_LIMIT and r["max_noise_coordinate"] < 2.0 ** 31


# ---- texture_value<double> == the reference's Texture.value, bit for bit -------------------------------
def test_texture_value_equals_every_kat_bit_for_bit():
    k = tb.kats()
    ks = tb.KatScene()
    assert len(k["textures"]) == 8 and {t["type"] for t in k["textures"]} == set(tb.TEX_CODE)
    for i, t in enumerate(k["textures"]):
        pts, want = np.array(t["points"], dtype=np.float64), np.array(t["values"], dtype=np.float64)
        assert len(pts) >= 200
        got = tb.host_texture_values(ks.desc, i, pts)
        bad = np.flatnonzero((tb.bits(got) != tb.bits(want)).any(axis=1))
        assert bad.size == 0, (t["type"], t["scale"], pts[bad[:3]], got[bad[:3]], want[bad[:3]])


def test_textured_scatter_equals_kats():
    """TexturedLambertian / TexturedMetal.scatter: result, attenuation and draws consumed (shade_segment's
    textured path on the given hit record); the SolidColor forms through their lowered plain materials."""
    k = tb.kats()
    solids = []
    for s in k["scatter"]:
        m = s["material"]
        if "solid" in m:
            key = (m["type"], tuple(m["solid"]), m.get("roughness", 0.0))
            if key not in solids:
                solids.append(key)
    code = {"lambertian": capi.RT_MAT_LAMBERTIAN, "metal": capi.RT_MAT_METAL}
    extra = [(capi.RT_MAT_METAL, (0, 0, 0), 1.0, 0)] + [(code[t], alb, r, -1) for t, alb, r in solids]
    ks = tb.KatScene(extra)
    nt = len(k["textures"])
    dp = C.POINTER(C.c_double)
    seen = set()
    for s in k["scatter"]:
        m = s["material"]
        if "solid" in m:
            mat = 2 * nt + 1 + solids.index((m["type"], tuple(m["solid"]), m.get("roughness", 0.0)))
        elif m["type"] == "metal" and m["roughness"] == 1:
            mat = 2 * nt
        else:
            mat = 2 * m["texture"] + (1 if m["type"] == "metal" else 0)
            assert m["type"] == "lambertian" or m["roughness"] == 0.35
        arr = lambda v: (C.c_double * 3)(*v)
        sc, out, draws = C.c_int(-1), (C.c_double * 9)(), C.c_uint(0)
        rc = tb.lib().ptx_scatter(C.byref(ks.desc), mat, arr(s["d"]), arr(s["point"]), arr(s["normal"]), int(s["frontFace"]),
                                  s["seed"], s["pixel"], s["sample"], C.byref(sc), out, C.byref(draws))
        assert rc == 0
        assert draws.value == s["draws"]
        assert s["emitted"] == [0, 0, 0]
        assert bool(sc.value) == (s["result"] is not None)
        seen.add((m["type"], s["result"] is not None))
        if s["result"] is not None:
            want = np.array(s["result"]["origin"] + s["result"]["dir"] + s["result"]["attenuation"], dtype=np.float64)
            assert np.array_equal(tb.bits(np.array(out[:])), tb.bits(want)), (m, list(out), want)
    assert ("metal", False) in seen and ("metal", True) in seen and ("lambertian", True) in seen


# ---- the sample-order CPU render of the three cases == the reference's -------------------------------
@pytest.mark.parametrize("case", tb.CASES)
@pytest.mark.parametrize("accel", [capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH], ids=["brute", "bvh"])
def test_cpu_sample_order_render_is_the_references(case, accel):
    rt, c = tb.tracer_for(case)
    rt.accel = accel
    p = rt.packed()
    assert p.num_textures > 0
    r = tb.host_render(p, rt.settings(crop=c["crop"]))
    lin = tb.load_array(case, "linear")
    assert not np.isnan(lin).any()
    assert np.array_equal(r["segments"], tb.load_array(case, "segs"))
    assert np.array_equal(r["draws"], tb.load_array(case, "draws"))
    same = tb.bits(r["mean"]) == tb.bits(lin)
    print(f"{case}: {same.mean():.4f} of channels bit-identical")
    assert same.all()


# ---- the three loaders agree, and equal what packing the real reference objects gave ------------------
def _py_pack(case):
    rt, c = tb.tracer_for(case)
    p = rt.packed()
    texs = [{"type": t.type, "perm": t.perm, "scale": t.scale, "odd": list(t.odd), "even": list(t.even)}
            for t in p.textures[:p.num_textures]]
    return {"textures": texs, "materialTexture": [int(x) for x in p.material_texture[:p.num_materials]],
            "texturePerms": [int(x) for x in p.texture_perms[:p.num_texture_perms].ravel()]}, p, c


def _cpp_pack(lib, c):
    src = open(scene_path(c["scene"]), "rb").read()
    h = C.c_void_p()
    capi.check(lib.rt_json_scene_load(src, len(src), c["requested"][0], c["requested"][1], c["seed"], C.byref(h)), lib)
    d = lib.rt_json_scene_desc(h).contents
    texs = [{"type": t.type, "perm": t.perm, "scale": t.scale, "odd": list(t.odd), "even": list(t.even)}
            for t in d.textures[:d.num_textures]]
    out = {"textures": texs, "materialTexture": list(d.material_texture[:d.num_materials]),
           "texturePerms": list(d.texture_perms[:512 * d.num_texture_perms])}
    mats = bytes(C.string_at(d.materials, 72 * d.num_materials))
    lib.rt_json_scene_destroy(h)
    return out, mats


@needs_node
@pytest.mark.parametrize("case", tb.CASES)
def test_three_loaders_agree_with_the_packed_reference_objects(lib, case):
    py, p, c = _py_pack(case)
    ref = c["packed"]
    want = {k: ref[k] for k in ("textures", "materialTexture", "texturePerms")}
    assert len(want["textures"]) > 0 and any(t >= 0 for t in want["materialTexture"])
    assert py == want
    cpp, cpp_mats = _cpp_pack(lib, c)
    assert cpp == want
    js = run_tool("pack", c["scene"], str(c["requested"][0]), str(c["requested"][1]), str(c["seed"]))
    assert {k: js[k] for k in want} == want
    # one material per object in all three, byte for byte
    assert base64.b64decode(js["materials"]) == cpp_mats == bytes(C.string_at(p.materials, 72 * p.num_materials))
    assert ref["numMaterials"] == p.num_materials


def test_texture_key_is_ignored_where_the_extension_says_so(lib):
    """tex_kitchen_sink: a `texture` on a dielectric, on an object the loader drops (its noise texture must not
    take a permutation index) and an unknown texture type (solid: the plain material)."""
    py, p, c = _py_pack("tex_kitchen_sink")
    assert [t["type"] for t in py["textures"]] == [capi.RT_TEX_MARBLE, capi.RT_TEX_WOOD, capi.RT_TEX_NOISE, capi.RT_TEX_CHECKER]
    assert [t["perm"] for t in py["textures"]] == [0, 1, 2, -1]
    assert py["materialTexture"] == [0, 1, 2, 3, -1, -1, -1]
    assert p.materials[5].type == capi.RT_MAT_DIELECTRIC
    assert list(p.materials[6].albedo) == [0.3, 0.8, 0.4]
    k = [texture_permutation(c["seed"], i) for i in range(3)]
    assert py["texturePerms"] == k[0] + k[1] + k[2]


def test_scenes_without_the_key_load_as_before():
    for name in ("sample_scene.json", "kitchen_sink.json", "cornell.json"):
        w, cam, _ = load_from_json(load_scene_json(name), 64, 48, permutation(1), keyed_texture_permutation(1))
        p = PackedScene(w, cam)
        assert p.num_textures == 0 and p.num_texture_perms == 0
        assert all(len(m) <= 3 for _, m, _ in w.objects)


# ---- texturePermutation: JS == Python == C++, and not the world's table -------------------------------
@needs_node
def test_texture_permutation_agrees_across_hosts(lib):
    seed = 12
    js = run_tool("perms", str(seed), "0", "1", "2", "4000000000")
    assert js["world"] == permutation(seed)
    for k, p in zip((0, 1, 2, 4000000000), js["textures"]):
        assert p == texture_permutation(seed, k)
        assert sorted(p[:256]) == list(range(256)) and p[256:] == p[:256]
        assert p != permutation(seed)
    assert texture_permutation(seed, 0) != texture_permutation(seed, 1)
    # C++: the loader's tables for the three noise-bearing textures of tex_kitchen_sink (seed 12)
    cpp, _ = _cpp_pack(lib, tb.manifest()["cases"]["tex_kitchen_sink"])
    assert cpp["texturePerms"] == sum((texture_permutation(seed, k) for k in range(3)), [])


# ---- pack.mjs: twins, reference-shaped objects, lowering, edits ---------------------------------------
@needs_node
def test_pack_mjs_packs_reference_shaped_textured_materials():
    d = run_tool("shapes")
    types = [t["type"] for t in d["textures"]]
    assert types == [capi.RT_TEX_CHECKER, capi.RT_TEX_MARBLE, capi.RT_TEX_WOOD]      # first appearance, by identity
    assert [t["perm"] for t in d["textures"]] == [-1, 0, 1]
    assert d["textures"][0]["scale"] == 4 and d["textures"][0]["odd"] == [0.1, 0.1, 0.1]
    # materials by identity: shared (twice the same object), metal checker, marble, mesh material, dielectric
    assert d["materialTexture"] == [0, 0, 1, 2, -1]
    assert d["texturePerms"] == texture_permutation(3, 0) + texture_permutation(3, 1)
    mats = np.frombuffer(base64.b64decode(d["materials"]), dtype=np.uint8).reshape(-1, 72)
    assert [int(m[:4].view(np.int32)[0]) for m in mats] == [capi.RT_MAT_LAMBERTIAN, capi.RT_MAT_METAL, capi.RT_MAT_LAMBERTIAN,
                                                            capi.RT_MAT_METAL, capi.RT_MAT_DIELECTRIC]


@needs_node
def test_constant_textures_lower_to_the_plain_material():
    d = run_tool("lowering")
    assert d["textured"]["textures"] == [] and d["textured"]["texturePerms"] == []
    assert d["textured"]["materialTexture"] == [-1, -1, -1]
    assert d["textured"] == d["plain"]                       # byte-identical records


@needs_node
def test_scene_change_detection_sees_a_texture_edit():
    d = run_tool("edit")
    assert d["texturesSame"] is False and d["materialsSame"] is True


def test_python_lowering_and_no_textures_for_plain_worlds():
    w, cam = default_scene(32, 24, permutation(0))
    p = PackedScene(w, cam)
    assert p.num_textures == 0 and p.desc.num_textures == 0 and p.desc.num_texture_perms == 0


# ---- rt_scene_create's host validation rejects bad texture descriptors --------------------------------
def _textured_world():
    w = World(permutation(3), keyed_texture_permutation(3))
    w.add("sphere", ("lambertian", (0.0, 0.0, 0.0), ("checker", 10.0, (0.1, 0.1, 0.1), (0.9, 0.9, 0.9))), ((0.0, 0.0, -1.0), 0.5))
    w.add("sphere", ("metal", (0.0, 0.0, 0.0), 0.2, ("marble", 2.0, w.new_texture_perm())), ((1.0, 0.0, -1.0), 0.5))
    w.add("sphere", ("dielectric", 1.5), ((2.0, 0.0, -1.0), 0.5))
    return w, default_scene(32, 24, permutation(3))[1]


def _mutations():
    def m(name, f, word):
        return pytest.param(f, word, id=name)
    return [
        m("texture index past the end", lambda p: p.material_texture.__setitem__(0, 2), "texture index"),
        m("texture index below -1", lambda p: p.material_texture.__setitem__(0, -2), "texture index"),
        m("texture on a dielectric", lambda p: p.material_texture.__setitem__(2, 0), "Lambertian / Metal"),
        m("texture on an emissive", lambda p: (setattr(p.materials[0], "type", capi.RT_MAT_EMISSIVE)), "Lambertian / Metal"),
        m("perm index past the end", lambda p: setattr(p.textures[1], "perm", 1), "perm index"),
        m("perm index on a checker", lambda p: setattr(p.textures[0], "perm", 0), "perm index"),
        m("negative perm index", lambda p: setattr(p.textures[1], "perm", -1), "perm index"),
        m("perm entry 256", lambda p: p.texture_perms.__setitem__((0, 511), 256), "texture_perms"),
        m("negative perm entry", lambda p: p.texture_perms.__setitem__((0, 7), -1), "texture_perms"),
        m("infinite scale", lambda p: setattr(p.textures[0], "scale", float("inf")), "scale"),
        m("NaN scale", lambda p: setattr(p.textures[1], "scale", float("nan")), "scale"),
        m("unknown texture type", lambda p: setattr(p.textures[0], "type", 4), "type"),
        m("negative texture count", lambda p: setattr(p.desc, "num_textures", -1), "textures"),
        m("textures pointer missing", lambda p: setattr(p.desc, "textures", None), "textures"),
        m("material_texture missing", lambda p: setattr(p.desc, "material_texture", None), "material_texture"),
    ]


@pytest.mark.parametrize("mutate,word", _mutations())
def test_invalid_texture_descriptors_are_rejected(lib, mutate, word):
    """Each invalid descriptor of the ABI: RT_ERR_INVALID with a message from rt_scene_create, on any machine
    (the texture checks run before the device is looked for), and from the shared host validation itself."""
    w, cam = _textured_world()
    p = PackedScene(w, cam)
    err = C.create_string_buffer(256)
    assert tb.lib().ptx_validate(C.byref(p.desc), err, 256) == 0, err.value
    mutate(p)
    assert tb.lib().ptx_validate(C.byref(p.desc), err, 256) == -1
    assert word in err.value.decode()
    h = C.c_void_p()
    assert lib.rt_scene_create(C.byref(p.desc), 0, C.byref(h)) == -1
    assert word in lib.rt_last_error().decode()


# ---- the descriptor says whether the texture fields are there ----------------------------------------
def test_descriptor_without_texture_fields_is_still_accepted(lib):
    """rt_abi_version() and rt_scene_desc.abi_version stay RT_ABI_VERSION: the texture fields are an append-only
    extension that a descriptor declares with extensions = RT_DESC_TEXTURES (formerly padding).  Any other
    value there means the struct ends at `perm`: nothing behind it is read, whatever lies there (a caller built
    against the shorter struct), and the scene is a plain one."""
    assert lib.rt_abi_version() == capi.RT_ABI_VERSION == 3
    w, cam = _textured_world()
    p = PackedScene(w, cam)
    assert p.desc.abi_version == capi.RT_ABI_VERSION and p.desc.extensions == capi.RT_DESC_TEXTURES
    err = C.create_string_buffer(256)
    pts = np.zeros((1, 3))
    dp = C.POINTER(C.c_double)
    assert tb.lib().ptx_texture_values(C.byref(p.desc), capi.RT_PREC_F64, 0, pts.ctypes.data_as(dp), 1, pts.ctypes.data_as(dp)) == 0
    for pad in (0, 1, -1, 0x54455833):                                          # what padding may hold
        p.desc.extensions = pad
        p.desc.num_textures = -7                                                # garbage behind perm: never read
        p.desc.num_texture_perms = 1 << 30
        p.desc.textures = C.cast(C.c_void_p(8), C.POINTER(capi.TextureDesc))
        p.desc.material_texture = C.cast(C.c_void_p(8), C.POINTER(C.c_int32))
        p.desc.texture_perms = C.cast(C.c_void_p(8), C.POINTER(C.c_int32))
        assert tb.lib().ptx_validate(C.byref(p.desc), err, 256) == 0, err.value
        assert tb.lib().ptx_texture_values(C.byref(p.desc), capi.RT_PREC_F64, 0, pts.ctypes.data_as(dp), 1, pts.ctypes.data_as(dp)) == -1
        h = C.c_void_p()
        rc = lib.rt_scene_create(C.byref(p.desc), 0, C.byref(h))
        assert rc in (0, -5), lib.rt_last_error()      # created, or no device here: never RT_ERR_INVALID
        if rc == 0:
            lib.rt_scene_destroy(h)
    p.desc.extensions = capi.RT_DESC_TEXTURES                                   # declared: the garbage is read and refused
    assert lib.rt_scene_create(C.byref(p.desc), 0, C.byref(h)) == -1


def test_texture_desc_layout_matches_c_compiler(tmp_path):
    """sizeof / offsetof of rt_texture_desc as gcc lays it out == the ctypes mirror (64 bytes, pack.mjs TEXTURE_BYTES)."""
    header = os.path.join(ROOT, "include", "rt_hip.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(rt_texture_desc));']
    for f in capi.TextureDesc._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(rt_texture_desc, {f[0]}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines() if l)
    assert int(got["size"]) == C.sizeof(capi.TextureDesc) == 64
    for f in capi.TextureDesc._fields_:
        assert int(got[f[0]]) == getattr(capi.TextureDesc, f[0]).offset, f[0]
