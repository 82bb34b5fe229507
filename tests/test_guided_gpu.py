"""The feature buffers (aov_kernel) and the guided filter (guided_level_kernel, csrc/pt_guided.hip) on the GPU:
bit for bit against tests/guided_ref.py and the CPU build of the same per-pixel code, then the guided epilogue
of rt_render / rt_finalize_device and how it meets checkpoints, resumes, crops and several devices."""
import ctypes as C

import numpy as np
import pytest

import epilogue_ref as er
import guided_ref as gr
import guidedcheck_binding as gb
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GUIDED_LEVELS, GUIDED_SIGMAS, GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
from test_guided import AOV_SCENES, INF, ref_levels

pytestmark = pytest.mark.gpu

DEFAULT_SIGMAS = (GUIDED_SIGMAS["color"], GUIDED_SIGMAS["albedo"], GUIDED_SIGMAS["normal"], GUIDED_SIGMAS["depth"])
RENDER_SCENES = ("sample_scene", "cornell", "sample_mesh")


@pytest.fixture(scope="module")
def scene(gpu):
    """Any scene: rt_guided_filter_device takes the frame from its arguments."""
    rt = GpuRayTracer(8, 8, seed=1)
    yield rt.scene_handle()
    rt.close()


def device_filter(scene, color, guides, levels, sigmas, twice=False):
    """rt_guided_filter_device on torch device tensors -> (out, the input buffer read back[, a second out])."""
    import torch
    lib = capi.load_library()
    h, w = color.shape[:2]
    d_color = torch.from_numpy(np.ascontiguousarray(color, dtype=np.float64)).cuda()
    d_guides = torch.from_numpy(np.ascontiguousarray(guides, dtype=np.float32)).cuda()
    p = gb.params(levels, sigmas)
    outs = []
    for _ in range(2 if twice else 1):
        d_out = torch.full((h, w, 3), -7.0, dtype=torch.float64, device="cuda")
        capi.check(lib.rt_guided_filter_device(scene, w, h, C.byref(p), C.c_void_p(d_color.data_ptr()),
                                               C.c_void_p(d_guides.data_ptr()), C.c_void_p(d_out.data_ptr()), None))
        torch.cuda.synchronize()
        outs.append(d_out.cpu().numpy())
    return (outs[0], d_color.cpu().numpy(), *outs[1:])


# ---- the filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", gr.FRAME_SIZES, ids=[f"{w}x{h}" for w, h in gr.FRAME_SIZES])
def test_device_filter_equals_reference(scene, w, h):
    """The frames of the CPU test (NaN, +inf, negative pixels, a row of misses, guide edges on and off a colour
    edge) at every level count; twice the same bits; the input is left as it was."""
    color, guides = gr.frame(w, h)
    ref = ref_levels(w, h)
    for levels in range(1, 9):
        out, kept, again = device_filter(scene, color, guides, levels, gr.SIGMAS, twice=True)
        assert gr.same(out, ref[levels - 1]), (levels, int(np.count_nonzero(gr.bits(out) != gr.bits(ref[levels - 1]))))
        assert gr.same(again, out) and gr.same(kept, color), levels


@pytest.mark.parametrize("which", range(4), ids=["color", "albedo", "normal", "depth"])
def test_device_filter_each_sigma_infinite(scene, which):
    sigmas = tuple(INF if k == which else s for k, s in enumerate(gr.SIGMAS))
    color, guides = gr.frame(17, 9)
    ref = gr.filter_levels(color, guides, 3, sigmas)
    for levels in (1, 3):
        assert gr.same(device_filter(scene, color, guides, levels, sigmas)[0], ref[levels - 1]), levels


def test_device_filter_refuses_in_place_and_misaligned_guides(scene):
    import torch
    lib = capi.load_library()
    d = torch.zeros(4 * 4 * 3 + 4 * 4 * 8 + 1, dtype=torch.float64, device="cuda")
    p = gb.params(2, gr.SIGMAS)
    ptr = lambda off: C.c_void_p(d.data_ptr() + off)                            # noqa: E731
    assert lib.rt_guided_filter_device(scene, 4, 4, C.byref(p), ptr(0), ptr(384), ptr(0), None) == -1
    assert lib.rt_guided_filter_device(scene, 4, 4, C.byref(p), ptr(0), ptr(388), ptr(1024), None) == -1


# ---- the feature buffers --------------------------------------------------------------------------------
def tracer(name, precision=capi.RT_PREC_F64, accel=capi.RT_ACCEL_AUTO, w=64, h=48, seed=3, **kw):
    rt = GpuRayTracer(w, h, seed=seed, precision=precision, accel=accel, **kw)
    assert rt.load_from_json(load_scene_json(name + ".json"))
    return rt


def guides_of(aov):
    """render_aovs' arrays as guide records (h, w, 8)"""
    h, w = aov["depth"].shape
    g = np.zeros((h, w, 8), dtype=np.float32)
    g[..., 0:3], g[..., 3:6], g[..., 6] = aov["albedo"], aov["normal"], aov["depth"]
    return g


def device_reference_aovs(rt, accel):
    """guided_ref.aovs with the closest hits of the device's own query (rt_closest_hits)."""
    lib = capi.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def hits(rays):
        n = len(rays)
        t, kind, idx = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        capi.check(lib.rt_closest_hits(rt.scene_handle(), rt.precision, accel, rays.ctypes.data_as(dp), n,
                                       t.ctypes.data_as(dp), kind.ctypes.data_as(ip), idx.ctypes.data_as(ip)))
        return t, kind, idx

    def tex(t, pts):
        # binary64: the device's own rt_texture_values (the albedo buffer calls the trace kernels' texture_value);
        # binary32: the albedo buffer's pinned-sine form (pt_path.h aov_texture_value) from the CPU build
        if rt.precision == capi.RT_PREC_F32:
            return gb.host_texture_values(rt.packed().desc, t, pts, precision=rt.precision)
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        rgb = np.zeros_like(pts)
        capi.check(lib.rt_texture_values(rt.scene_handle(), rt.precision, t, pts.ctypes.data_as(dp), len(pts),
                                         rgb.ctypes.data_as(dp)))
        return rgb

    return gr.aovs(rt.packed().desc, rt.width, rt.height, rt.precision, hits, tex)


@pytest.mark.parametrize("precision", [capi.RT_PREC_F64, capi.RT_PREC_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", AOV_SCENES)
def test_device_aovs_equal_cpu_build_and_reference(gpu, name, precision):
    """rt_aovs in World order and through the trees: identical bits, equal to the CPU build of aov_pixel, and
    to guided_ref on rt_closest_hits' own hits (so kind, index and t are that query's).

    Binary32 textured albedo is the same bits on the GPU and in the CPU build because aov_texture_value takes
    its sine from V8's binary64 Math.sin rounded to binary32, not from the platform's sinf (with sinf, 304 of
    tex_mesh_wood_crop's 24576 values differed by 1 ulp between the device's library and the C library)."""
    got = {}
    for accel in (capi.RT_ACCEL_BRUTE, capi.RT_ACCEL_BVH):
        rt = tracer(name, precision, accel)
        aov = rt.render_aovs()
        st = rt.settings()
        cpu_g, cpu_kind, cpu_idx = gb.host_aovs(rt.packed(), st)
        g = guides_of(aov)
        ref_g, ref_kind, ref_idx = device_reference_aovs(rt, accel)
        for label, other in (("CPU build", cpu_g), ("guided_ref on the device's hits", ref_g)):
            diff = gr.bits(g) != gr.bits(other)
            ulps = np.abs(gr.bits(g).astype(np.int64) - gr.bits(other).astype(np.int64))[diff]
            print(f"{name} {'f32' if precision else 'f64'} accel {accel} vs {label}: {int(diff.sum())} of {diff.size} values "
                  f"differ, fields {sorted(set(np.nonzero(diff)[2].tolist()))}, at most {int(ulps.max()) if ulps.size else 0} ulp")
        assert gr.same(g, cpu_g), (accel, int(np.count_nonzero(gr.bits(g) != gr.bits(cpu_g))))
        assert np.array_equal(aov["kind"], cpu_kind) and np.array_equal(aov["index"], cpu_idx)
        assert gr.same(g, ref_g) and np.array_equal(aov["kind"], ref_kind) and np.array_equal(aov["index"], ref_idx)
        got[accel] = (g, aov["kind"], aov["index"])
        rt.close()
    a, b = got[capi.RT_ACCEL_BRUTE], got[capi.RT_ACCEL_BVH]
    assert gr.same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("precision", [capi.RT_PREC_F64, capi.RT_PREC_F32], ids=["f64", "f32"])
def test_device_aovs_through_the_grid_walk(gpu, precision):
    """RTOW's launches walk the uniform grid with its records in LDS: the staged form of aov_kernel."""
    rt = tracer("rtow", precision, w=48, h=27)
    lib = capi.load_library()
    assert lib.rt_scene_walk(rt.scene_handle(), precision, capi.RT_ACCEL_AUTO) == 2
    aov = rt.render_aovs()
    cpu_g, cpu_kind, cpu_idx = gb.host_aovs(rt.packed(), rt.settings())
    assert gr.same(guides_of(aov), cpu_g) and np.array_equal(aov["kind"], cpu_kind) and np.array_equal(aov["index"], cpu_idx)
    crop = (5, 3, 17, 11)
    part = rt.render_aovs(crop=crop)
    assert gr.same(guides_of(part), cpu_g[3:14, 5:22])
    rt.close()
    brute = tracer("rtow", precision, capi.RT_ACCEL_BRUTE, w=48, h=27)
    assert gr.same(guides_of(brute.render_aovs()), cpu_g)
    brute.close()


def test_render_returns_the_feature_buffers(gpu):
    rt = tracer("sample_scene")
    res = rt.render(want=("mean", "albedo", "normal", "depth"))
    aov = rt.render_aovs()
    assert all(gr.same(res[k], aov[k]) for k in ("albedo", "normal", "depth"))
    rt.close()


def test_aovs_device_writes_the_guide_records(gpu):
    import torch
    rt = tracer("kitchen_sink")
    d = torch.full((48, 64, 8), -1.0, dtype=torch.float32, device="cuda")
    capi.check(capi.load_library().rt_aovs_device(rt.scene_handle(), C.byref(rt.settings()), C.c_void_p(d.data_ptr()), None))
    torch.cuda.synchronize()
    assert gr.same(d.cpu().numpy(), guides_of(rt.render_aovs()))
    rt.close()


# ---- the guided render ------------------------------------------------------------------------------------
_renders = {}


def renders(name):
    """(plain render, guided render, guides) of a scene at 64 x 48, 4 spp, f64, computed once."""
    if name not in _renders:
        rt = tracer(name)
        rt.update_render_settings({"samples": 4})
        plain = rt.render(want=("mean",))
        guides = guides_of(rt.render_aovs())
        rt.update_render_settings({"samples": 4, "guidedDenoise": True})
        guided = rt.render(want=("mean",))
        rt.close()
        _renders[name] = (plain, guided, guides)
    return _renders[name]


def check_epilogue_of(mean, st, post, rgba8, label):
    """post and rgba8 are tests/epilogue_ref.py's of `mean` (one sample): the Float32 frame is one of the two
    nearest binary32 values of the exact power, a byte is floor(255 p) unless 255 p is within 3 ulps of an integer."""
    tone = {capi.RT_TM_ACES: "aces", capi.RT_TM_LINEAR: "linear"}.get(st.tone_map, "reinhard")
    _, tm = er.stage_a(tone, st.exposure, 1, mean.ravel())
    lo, hi, want, exempt, k = er.stage_b(st.gamma, tm)
    p32 = post[..., :3].ravel()
    nan = np.isnan(lo)
    assert not np.where(nan, ~np.isnan(p32), (p32 != lo) & (p32 != hi)).any(), label
    byte = rgba8[..., :3].ravel().astype(np.int64)
    assert not ((byte != want) & ~(exempt & ((byte == k - 1) | (byte == k)))).any(), label
    assert (post[..., 3] == 1.0).all() and (rgba8[..., 3] == 255).all(), label


@pytest.mark.parametrize("name", RENDER_SCENES)
def test_guided_render_is_the_reference_filter_of_the_plain_mean(gpu, name):
    plain, guided, guides = renders(name)
    ref = gr.guided_filter(plain["mean"], guides, GUIDED_LEVELS, DEFAULT_SIGMAS)
    assert gr.same(guided["mean"], ref), int(np.count_nonzero(gr.bits(guided["mean"]) != gr.bits(ref)))
    assert not gr.same(guided["mean"], plain["mean"])
    rt = tracer(name)
    rt.update_render_settings({"samples": 4})
    check_epilogue_of(ref, rt.settings(), guided["post"], guided["rgba8"], name)
    rt.close()


@pytest.mark.parametrize("name", RENDER_SCENES)
def test_guided_render_with_the_gaussian_denoise_after_it(gpu, name):
    """denoising on: the same filtered mean, and the frame equals the unguided epilogue (finalize + denoise,
    tests/test_epilogue_gpu.py) of that filtered mean as one-sample sums."""
    _, guided, _ = renders(name)
    rt = tracer(name)
    rt.update_render_settings({"samples": 4, "denoising": True, "denoiseStrength": 0.8, "guidedDenoise": True})
    both = rt.render(want=("mean",))
    assert gr.same(both["mean"], guided["mean"])
    rt.close()
    off = tracer(name)                               # a scene without the filter: the plain epilogue
    off.update_render_settings({"samples": 1, "denoising": True, "denoiseStrength": 0.8})
    dev = er.finalize_device(off.scene_handle(), off.settings(), guided["mean"], post=True)
    off.close()
    assert gr.same(both["post"].reshape(-1, 4), dev["post"]) and np.array_equal(both["rgba8"].reshape(-1, 4), dev["rgba8"])
    assert not np.array_equal(both["rgba8"], guided["rgba8"])


def test_guided_and_the_rest_of_the_boundary(gpu):
    plain, guided, _ = renders("sample_scene")
    rt = tracer("sample_scene")
    rt.update_render_settings({"samples": 4, "guidedDenoise": True})
    with pytest.raises(RuntimeError, match="INVALID"):
        rt.render(crop=(3, 2, 20, 10))
    again = rt.render(want=("mean",))
    assert gr.same(again["mean"], guided["mean"]) and np.array_equal(again["rgba8"], guided["rgba8"])
    sums, done = rt.checkpoint()                     # the raw sums, never the filtered frame
    assert done == 4 and gr.same(sums / 4.0, plain["mean"])
    one = rt.render(want=("mean",), batch_samples=2)          # the same batches on one device and dealt to two
    two = rt.render(want=("mean",), batch_samples=2, devices=[0, 0])
    assert gr.same(two["mean"], one["mean"]) and np.array_equal(two["rgba8"], one["rgba8"])
    assert gr.same(two["post"], one["post"])
    rt.update_render_settings({"samples": 4, "guidedDenoise": False})
    off = rt.render(want=("mean",))
    assert gr.same(off["mean"], plain["mean"]) and np.array_equal(off["rgba8"], plain["rgba8"])
    assert gr.same(off["post"], plain["post"])
    rt.close()


def test_cancelled_and_resumed_guided_render_equals_the_one_batch_render(gpu):
    """Sample-order sums (batches then add exactly as one launch does): cancel after the first batch (the three
    queued behind it complete), resume in a new scene from the checkpoint — the raw sums — and the guided frame
    is the uninterrupted one's."""
    def make():
        rt = tracer("cornell", sum_order=capi.RT_SUM_SAMPLE_ORDER)
        rt.update_render_settings({"samples": 8, "guidedDenoise": True})
        return rt
    rt = make()
    whole = rt.render(want=("mean",))
    with pytest.raises(RuntimeError, match="CANCELLED"):
        rt.render(batch_samples=1, on_progress=lambda f: True)
    sums, done = rt.checkpoint()
    assert 1 <= done < 8
    rt.close()
    rt2 = make()
    res = rt2.render(want=("mean",), resume=(sums, done), batch_samples=1)
    assert gr.same(res["mean"], whole["mean"]) and np.array_equal(res["rgba8"], whole["rgba8"])
    assert gr.same(res["post"], whole["post"])
    rt2.close()


def test_finalize_device_on_traced_sums_gives_the_renders_bytes(gpu):
    import torch
    _, guided, _ = renders("sample_mesh")
    rt = tracer("sample_mesh")
    rt.update_render_settings({"samples": 4, "guidedDenoise": True})
    lib = capi.load_library()
    scene = rt.scene_handle()
    rt._apply_guided(lib, scene)
    st = rt.settings()
    n = 64 * 48
    d_sum = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    capi.check(lib.rt_trace_device(scene, C.byref(st), C.c_void_p(d_sum.data_ptr()), None, 1, None))
    kept = d_sum.clone()
    d_mean = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    d_post = torch.zeros(4 * n, dtype=torch.float32, device="cuda")
    d_rgba = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731
    capi.check(lib.rt_finalize_device(scene, C.byref(st), ptr(d_sum), ptr(d_mean), ptr(d_post), ptr(d_rgba), None))
    torch.cuda.synchronize()
    assert torch.equal(kept, d_sum)
    assert gr.same(d_mean.cpu().numpy().reshape(48, 64, 3), guided["mean"])
    assert gr.same(d_post.cpu().numpy().reshape(48, 64, 4), guided["post"])
    assert np.array_equal(d_rgba.cpu().numpy().reshape(48, 64, 4), guided["rgba8"])
    d_only = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")              # the RGBA8-only call
    capi.check(lib.rt_finalize_device(scene, C.byref(st), ptr(d_sum), None, None, ptr(d_only), None))
    torch.cuda.synchronize()
    assert torch.equal(d_only, d_rgba)
    st.crop_x0, st.crop_y0, st.crop_w, st.crop_h = 0, 0, 32, 48
    assert lib.rt_finalize_device(scene, C.byref(st), ptr(d_sum), None, None, ptr(d_only), None) == -1
    rt.close()


# ---- quality: a condition on the defaults ----------------------------------------------------------------
def post_rms(a, b):
    d = np.clip(a[..., :3].astype(np.float64), 0, 1) - np.clip(b[..., :3].astype(np.float64), 0, 1)
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("name", RENDER_SCENES)
def test_guided_frame_is_closer_to_the_converged_frame(gpu, name):
    """Post-gamma RMS against a 1024-spp plain render of the same 64 x 48 frame (another seed): the guided 4-spp
    frame must be strictly below the plain 4-spp frame with the default parameters."""
    plain, guided, _ = renders(name)
    rt = tracer(name, seed=99)
    rt.update_render_settings({"samples": 1024})
    ref = rt.render()["post"]
    rt.close()
    e_plain, e_guided = post_rms(plain["post"], ref), post_rms(guided["post"], ref)
    print(f"{name}: post-gamma RMS vs 1024 spp: plain 4 spp {e_plain:.5f}, guided 4 spp {e_guided:.5f}, "
          f"ratio {e_guided / e_plain:.3f}")
    assert e_guided < e_plain


# ---- the other hosts ----------------------------------------------------------------------------------------
_NODE_SCRIPT = r'''
import fs from 'fs';
import { pathToFileURL } from 'url';
const [root, scenePath, out] = process.argv.slice(2);
(async () => {
const { GpuRayTracer } = await import(pathToFileURL(root + '/blenderraytracer_amd/js/gpu-ray-tracer.mjs').href);
const rt = new GpuRayTracer({ width: 64, height: 48 }, { seed: 3 });
if (!rt.loadFromJSON(JSON.parse(fs.readFileSync(scenePath, 'utf8')))) process.exit(3);
rt.updateRenderSettings({ samples: 4, guidedDenoise: true });
const kept = [rt.guidedDenoise, rt.guidedLevels];
rt.updateRenderSettings({ samples: 4 });                       // without the keys: the filter stays as it was
if (rt.guidedDenoise !== kept[0] || rt.guidedLevels !== kept[1]) process.exit(4);
const res = await rt.renderBuffers({});
fs.writeFileSync(out + '.rgba8', Buffer.from(res.rgba8.buffer, res.rgba8.byteOffset, res.rgba8.byteLength));
const aov = rt.renderAovs();
for (const k of ['albedo', 'normal', 'depth', 'kind', 'index']) {
    if (k !== 'kind' && k !== 'index' && !(aov[k] instanceof Float32Array)) process.exit(5);
    fs.writeFileSync(out + '.' + k, Buffer.from(aov[k].buffer, aov[k].byteOffset, aov[k].byteLength));
}
rt.updateRenderSettings({ samples: 4, guidedDenoise: false });
const plain = await rt.renderBuffers({});
fs.writeFileSync(out + '.plain', Buffer.from(plain.rgba8.buffer, plain.rgba8.byteOffset, plain.rgba8.byteLength));
})().catch((e) => { console.error(e); process.exit(1); });
'''


def test_node_guided_frame_and_aovs_equal_pythons(gpu, tmp_path):
    import os
    import shutil
    import subprocess
    from blenderraytracer_amd.scene import scene_path
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "blenderraytracer_amd", "lib", "rt_napi.node")), "rt_napi.node missing"
    script = tmp_path / "guided.mjs"
    script.write_text(_NODE_SCRIPT)
    out = str(tmp_path / "node")
    r = subprocess.run([node, str(script), root, scene_path("sample_scene.json"), out], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    plain, guided, guides = renders("sample_scene")
    assert np.array_equal(np.fromfile(out + ".rgba8", dtype=np.uint8).reshape(48, 64, 4), guided["rgba8"])
    assert np.array_equal(np.fromfile(out + ".plain", dtype=np.uint8).reshape(48, 64, 4), plain["rgba8"])
    assert gr.same(np.fromfile(out + ".albedo", dtype=np.float32).reshape(48, 64, 3), guides[..., 0:3])
    assert gr.same(np.fromfile(out + ".normal", dtype=np.float32).reshape(48, 64, 3), guides[..., 3:6])
    assert gr.same(np.fromfile(out + ".depth", dtype=np.float32).reshape(48, 64), guides[..., 6])
    rt = tracer("sample_scene")
    aov = rt.render_aovs()
    rt.close()
    assert np.array_equal(np.fromfile(out + ".kind", dtype=np.int32).reshape(48, 64), aov["kind"])
    assert np.array_equal(np.fromfile(out + ".index", dtype=np.int32).reshape(48, 64), aov["index"])


def read_pfm(path):
    """A PFM file -> (h, w[, 3]) float32, top-down; checks the header."""
    with open(path, "rb") as f:
        data = f.read()
    magic, dims, scale, body = data.split(b"\n", 3)
    assert magic in (b"PF", b"Pf") and float(scale) < 0            # little-endian
    w, h = (int(x) for x in dims.split())
    ch = 3 if magic == b"PF" else 1
    assert len(body) == 4 * w * h * ch
    a = np.frombuffer(body, dtype="<f4").reshape((h, w, 3) if ch == 3 else (h, w))
    return a[::-1]                                                 # PFM rows run bottom to top


def test_cli_guided_frame_and_aov_files_equal_pythons(gpu, tmp_path):
    import os
    import subprocess
    from blenderraytracer_amd.scene import scene_path
    from test_cli import CLI, read_pam
    assert os.path.exists(CLI), "rt_render_cli missing"
    out, prefix = tmp_path / "img.pam", str(tmp_path / "aov")
    args = [CLI, scene_path("sample_scene.json"), "--width", "64", "--height", "48", "--spp", "4", "--seed", "3"]
    r = subprocess.run(args + ["--guided", "--aovs", prefix, "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain, guided, guides = renders("sample_scene")
    assert np.array_equal(read_pam(out), guided["rgba8"])
    assert gr.same(np.ascontiguousarray(read_pfm(prefix + ".albedo.pfm")), guides[..., 0:3])
    assert gr.same(np.ascontiguousarray(read_pfm(prefix + ".normal.pfm")), guides[..., 3:6])
    assert gr.same(np.ascontiguousarray(read_pfm(prefix + ".depth.pfm")), guides[..., 6])
    sig = ",".join(repr(s) for s in DEFAULT_SIGMAS)
    r = subprocess.run(args + ["--guided-levels", str(GUIDED_LEVELS), "--guided-sigma", sig, "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and np.array_equal(read_pam(out), guided["rgba8"]), r.stderr
    r = subprocess.run(args + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and np.array_equal(read_pam(out), plain["rgba8"]), r.stderr
    r = subprocess.run(args + ["--guided-levels", "9"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "guided levels" in r.stderr
