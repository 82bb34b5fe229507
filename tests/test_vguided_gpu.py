"""The variance-guided form of the guided filter on the GPU (vguided_level_kernel, csrc/pt_guided.hip): bit for bit
against tests/vguided_ref.py for both outputs, then the variance-guided epilogue of rt_render and how it meets
the error estimate, checkpoints, resumes, crops, several devices and the noise-threshold stop."""
import ctypes as C

import numpy as np
import pytest

import guided_ref as gr
import guidedcheck_binding as gb
import vguided_ref as vr
from blenderraytracer_amd import capi
from blenderraytracer_amd.renderer import GUIDED_LEVELS, GUIDED_SIGMA_VARIANCE, GUIDED_SIGMAS, GpuRayTracer
from blenderraytracer_amd.scene import load_scene_json
from test_guided_gpu import check_epilogue_of, guides_of, post_rms
from test_vguided import INF, mismatches, ref_levels

pytestmark = pytest.mark.gpu

DEFAULT_SIGMAS = (GUIDED_SIGMAS["color"], GUIDED_SIGMAS["albedo"], GUIDED_SIGMAS["normal"], GUIDED_SIGMAS["depth"])
RENDER_SCENES = ("sample_scene", "cornell", "sample_mesh")
SPP, BATCH = 8, 4          # two batches of one chunk each: K = 2, the least the estimate allows


@pytest.fixture(scope="module")
def scene(gpu):
    """Any scene: rt_guided_filter_variance_device takes the frame from its arguments."""
    rt = GpuRayTracer(8, 8, seed=1)
    yield rt.scene_handle()
    rt.close()


def device_filter(scene, color, var, guides, levels, sigmas, sv, twice=False, want_var=True):
    """rt_guided_filter_variance_device on torch device tensors -> [(c', v')] per call, and the inputs read back."""
    import torch
    lib = capi.load_library()
    h, w = color.shape[:2]
    d_color = torch.from_numpy(np.ascontiguousarray(color, dtype=np.float64)).cuda()
    d_var = torch.from_numpy(np.ascontiguousarray(var, dtype=np.float64)).cuda()
    d_guides = torch.from_numpy(np.ascontiguousarray(guides, dtype=np.float32)).cuda()
    p = gb.params(levels, sigmas)
    outs = []
    for _ in range(2 if twice else 1):
        d_out = torch.full((h, w, 3), -7.0, dtype=torch.float64, device="cuda")
        d_vout = torch.full((h, w, 3), -7.0, dtype=torch.float64, device="cuda")
        capi.check(lib.rt_guided_filter_variance_device(
            scene, w, h, C.byref(p), float(sv), C.c_void_p(d_color.data_ptr()), C.c_void_p(d_var.data_ptr()),
            C.c_void_p(d_guides.data_ptr()), C.c_void_p(d_out.data_ptr()),
            C.c_void_p(d_vout.data_ptr()) if want_var else None, None))
        torch.cuda.synchronize()
        outs.append((d_out.cpu().numpy(), d_vout.cpu().numpy()))
    return outs, (d_color.cpu().numpy(), d_var.cpu().numpy(), d_guides.cpu().numpy())


# ---- the filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", gr.FRAME_SIZES, ids=[f"{w}x{h}" for w, h in gr.FRAME_SIZES])
def test_device_filter_equals_reference(scene, w, h):
    """The frames of the CPU test (40 x 24 spans 2 x 3 workgroups of 32 x 8) at every level count, both outputs;
    twice the same bits; the inputs are left as they were."""
    color, guides = gr.frame(w, h)
    var = vr.variance_frame(w, h)
    ref = ref_levels(w, h, 4.0)
    for levels in range(1, 9):
        outs, kept = device_filter(scene, color, var, guides, levels, gr.SIGMAS, 4.0, twice=True)
        (c, v), (c2, v2) = outs
        rc, rv = ref[levels - 1]
        assert gr.same(c, rc), ("colour", levels, mismatches(c, rc))
        assert gr.same(v, rv), ("variance", levels, mismatches(v, rv))
        assert gr.same(c2, c) and gr.same(v2, v), levels
        assert gr.same(kept[0], color) and gr.same(kept[1], var) and gr.same(kept[2], guides), levels


@pytest.mark.parametrize("w,h", gr.FRAME_SIZES, ids=[f"{w}x{h}" for w, h in gr.FRAME_SIZES])
def test_device_filter_with_infinite_sigma_variance(scene, w, h):
    """isv = 0: the colour term drops out on the device as in the reference (zero-variance pixels included)."""
    color, guides = gr.frame(w, h)
    var = vr.variance_frame(w, h)
    ref = vr.filter_levels(color, var, guides, 8, gr.SIGMAS, INF)
    for levels in range(1, 9):
        (c, v), = device_filter(scene, color, var, guides, levels, gr.SIGMAS, INF)[0]
        assert gr.same(c, ref[levels - 1][0]) and gr.same(v, ref[levels - 1][1]), levels


def test_device_filter_without_the_variance_output(scene):
    color, guides = gr.frame(40, 24)
    var = vr.variance_frame(40, 24)
    ref = ref_levels(40, 24, 4.0)
    for levels in (1, 2, 5):
        (c, v), = device_filter(scene, color, var, guides, levels, gr.SIGMAS, 4.0, want_var=False)[0]
        assert gr.same(c, ref[levels - 1][0]), levels
        assert (v == -7.0).all()                         # the buffer the call was not given stays untouched


def test_device_filter_refuses_overlaps_and_misaligned_guides(scene):
    import torch
    lib = capi.load_library()
    n = 4 * 4
    d = torch.zeros(5 * 3 * n + 8 * n, dtype=torch.float64, device="cuda")
    p = gb.params(2, gr.SIGMAS)
    ptr = lambda off: C.c_void_p(d.data_ptr() + off) if off is not None else None            # noqa: E731
    F = 24 * n                                           # one colour / variance frame in bytes
    color, var, guides, out, vout = 0, F, 2 * F, 2 * F + 32 * n, 3 * F + 32 * n

    def call(color, var, guides, out, vout):
        return lib.rt_guided_filter_variance_device(scene, 4, 4, C.byref(p), 4.0, ptr(color), ptr(var), ptr(guides), ptr(out),
                                                    ptr(vout), None)
    assert call(color, var, guides, out, vout) == 0
    assert call(color, var, guides, out, None) == 0
    torch.cuda.synchronize()
    for bad in [(color, var, guides, color, vout),       # in place: colour
                (color, var, guides, out, var),          # in place: variance
                (color, var, guides, var, vout),         # the colour output over the variance input
                (color, var, guides, out, color),        # the variance output over the colour input
                (color, var, guides, guides, vout),      # an output over the guides
                (color, var, guides, out, out),          # the two outputs on each other
                (color, var, guides, out, out + 8),      # ... partly
                (color, var, guides, color + F - 8, None),   # partial overlap with an input (last double of colour)
                (color, var, guides + 8, out + 8, None)]:    # misaligned guides
        assert call(*bad) == -1, bad
        assert b"overlap" in lib.rt_last_error() or b"aligned" in lib.rt_last_error()


# ---- the variance-guided render ---------------------------------------------------------------------------
def tracer(name, w=64, h=48, seed=3, estimate=True, **kw):
    rt = GpuRayTracer(w, h, seed=seed, error_estimate=estimate, **kw)
    assert rt.load_from_json(load_scene_json(name + ".json"))
    return rt


ON = {"guidedDenoise": True, "guidedVariance": True}
_renders = {}


def renders(name, spp=SPP, batch=BATCH):
    """Of a scene at 64 x 48, f64, seed 3, in batches: the plain render, its var_mean and guides, the plain guided
    render, the variance-guided render with its filtered variance, and the reference filter; computed once."""
    key = (name, spp, batch)
    if key not in _renders:
        rt = tracer(name)
        rt.update_render_settings({"samples": spp})
        plain = rt.render(want=("mean",), batch_samples=batch)
        var, _ = rt.error_estimate()
        groups = rt.error_stats()["groups"]
        guides = guides_of(rt.render_aovs())
        rt.update_render_settings({"samples": spp, "guidedDenoise": True})
        guided = rt.render(want=("mean",), batch_samples=batch)
        rt.update_render_settings({"samples": spp, **ON})
        vguided = rt.render(want=("mean",), batch_samples=batch)
        fvar = rt.filtered_variance()
        st = rt.settings()
        rt.close()
        ref = vr.vguided_filter(plain["mean"], var, guides, GUIDED_LEVELS, DEFAULT_SIGMAS, GUIDED_SIGMA_VARIANCE)
        _renders[key] = dict(plain=plain, var=var, groups=groups, guides=guides, guided=guided, vguided=vguided, fvar=fvar,
                             ref=ref, settings=st)
    return _renders[key]


@pytest.mark.parametrize("name", RENDER_SCENES)
def test_render_is_the_reference_filter_of_the_plain_mean_and_its_estimate(gpu, name):
    r = renders(name)
    assert r["groups"] == 2
    got, (rc, rv) = r["vguided"], r["ref"]
    assert gr.same(got["mean"], rc), mismatches(got["mean"], rc)
    assert not gr.same(got["mean"], r["plain"]["mean"]) and not gr.same(got["mean"], r["guided"]["mean"])
    check_epilogue_of(rc, r["settings"], got["post"], got["rgba8"], name)
    assert gr.same(r["fvar"], rv), mismatches(r["fvar"], rv)


def test_refused_before_tracing(gpu):
    """Without the guided filter, without the estimate, with one group, with a crop and from host sums: RT_ERR_INVALID,
    and nothing was traced — the scene's checkpoint of the render before is still there where the refusal comes
    before the render takes the scene over, and in every case no sample was added."""
    r = renders("sample_scene")
    rt = tracer("sample_scene")
    rt.update_render_settings({"samples": SPP, "guidedVariance": True})            # no guided filter
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID.*guided filter"):
        rt.render(batch_samples=BATCH)
    rt.update_render_settings({"samples": SPP, **ON})
    rt.error_estimate_on = False                                                   # no estimate
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID.*error estimate"):
        rt.render(batch_samples=BATCH)
    rt.error_estimate_on = True
    rt.update_render_settings({"samples": 4, **ON})                                # one batch of one chunk: 1 group
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID.*2 groups"):
        rt.render()
    assert rt.last_stats is None                                                   # no render has returned yet
    rt.update_render_settings({"samples": SPP, **ON})
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID.*full frame"):
        rt.render(batch_samples=BATCH, crop=(3, 2, 20, 10))
    ok = rt.render(want=("mean",), batch_samples=BATCH)
    assert gr.same(ok["mean"], r["vguided"]["mean"])
    sums, done = rt.checkpoint()                                                   # the raw sums, never the filtered frame
    assert done == SPP and gr.same(sums / float(SPP), r["plain"]["mean"])
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID.*host sums"):
        rt.render(batch_samples=BATCH, resume=(sums, BATCH))
    assert rt.checkpoint()[1] == SPP and gr.same(rt.checkpoint()[0], sums)         # that refusal touched nothing
    rt.close()


def test_finalize_device_is_refused_while_the_variance_form_is_on(gpu):
    import torch
    rt = tracer("sample_scene")
    rt.update_render_settings({"samples": 4, **ON})
    lib, scene = capi.load_library(), rt.scene_handle()
    rt._apply_guided(lib, scene)
    st = rt.settings()
    n = 64 * 48
    d_sum = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    d_rgba = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    args = (scene, C.byref(st), C.c_void_p(d_sum.data_ptr()), None, None, C.c_void_p(d_rgba.data_ptr()), None)
    assert lib.rt_finalize_device(*args) == -1 and b"estimate" in lib.rt_last_error()
    capi.check(lib.rt_scene_set_guided_variance(scene, 0.0))                       # off: the plain guided epilogue again
    capi.check(lib.rt_finalize_device(*args))
    torch.cuda.synchronize()
    rt.close()


def test_resume_devices_and_switching_off(gpu):
    r = renders("sample_scene")
    whole = r["vguided"]
    rt = tracer("sample_scene")
    rt.update_render_settings({"samples": SPP, **ON})
    with pytest.raises(RuntimeError, match="RT_ERR_INVALID"):                      # no variance-guided epilogue yet
        rt.filtered_variance()
    with pytest.raises(RuntimeError, match="CANCELLED"):                           # cancelled: unfiltered, as before
        rt.render(batch_samples=BATCH, on_progress=lambda f: True)
    done = rt.checkpoint()[1]
    assert 0 < done < SPP
    res = rt.render(want=("mean",), batch_samples=BATCH, resume=(None, done))      # resident: the moments continue
    for k in ("mean", "post", "rgba8"):
        assert gr.same(res[k], whole[k]) if k != "rgba8" else np.array_equal(res[k], whole[k]), k
    assert gr.same(rt.filtered_variance(), r["fvar"])
    two = rt.render(want=("mean",), batch_samples=BATCH, devices=[0, 0])
    assert gr.same(two["mean"], whole["mean"]) and gr.same(two["post"], whole["post"])
    assert np.array_equal(two["rgba8"], whole["rgba8"])
    rt.update_render_settings({"samples": SPP, "guidedVariance": False})           # the plain guided render's bits
    off = rt.render(want=("mean",), batch_samples=BATCH)
    assert gr.same(off["mean"], r["guided"]["mean"]) and np.array_equal(off["rgba8"], r["guided"]["rgba8"])
    assert gr.same(rt.filtered_variance(), r["fvar"])                              # still the last variance epilogue's
    rt.update_render_settings({"samples": SPP, "guidedDenoise": False})            # both off: the plain render's bits
    off = rt.render(want=("mean",), batch_samples=BATCH)
    assert gr.same(off["mean"], r["plain"]["mean"]) and np.array_equal(off["rgba8"], r["plain"]["rgba8"])
    assert gr.same(off["post"], r["plain"]["post"])
    rt.close()


def test_noise_threshold_stop_filters_the_committed_samples(gpu):
    spp, batch, nb = 32, 4, 8
    rt = tracer("cornell")
    rt.update_render_settings({"samples": spp})
    errs = []
    rt.render(batch_samples=batch, on_progress=lambda f: errs.append(rt.error_stats()["frame_error"]) and False)
    thr = errs[nb // 2 - 1]
    guides = guides_of(rt.render_aovs())
    rt.update_render_settings({"samples": spp, **ON})
    res = rt.render(want=("mean",), batch_samples=batch, noise_threshold=thr)
    st = rt.error_stats()
    sums, done = rt.checkpoint()
    assert st["converged"] == 1 and 2 * batch <= done == st["samples"] < spp and st["groups"] >= 2
    var, _ = rt.error_estimate()
    rc, rv = vr.vguided_filter(sums / float(done), var, guides, GUIDED_LEVELS, DEFAULT_SIGMAS, GUIDED_SIGMA_VARIANCE)
    assert gr.same(res["mean"], rc), mismatches(res["mean"], rc)
    assert gr.same(rt.filtered_variance(), rv)
    rt.close()


# ---- quality: a condition on the default --------------------------------------------------------------------
@pytest.mark.parametrize("name", RENDER_SCENES)
def test_variance_guided_frame_is_closer_to_the_converged_frame(gpu, name):
    """16 spp in four batches, post-gamma RMS against a 1024-spp plain render (seed 99) of the same 64 x 48 frame:
    strictly below the unfiltered frame's with the default sigma_variance."""
    rt = tracer(name)
    frames = {}
    for label, keys in (("plain", {}), ("guided", {"guidedDenoise": True}), ("variance", ON)):
        rt.update_render_settings({"samples": 16, "guidedDenoise": False, "guidedVariance": False, **keys})
        frames[label] = rt.render(batch_samples=4)["post"]
    assert rt.error_stats()["groups"] == 4
    rt.close()
    conv = tracer(name, seed=99, estimate=False)
    conv.update_render_settings({"samples": 1024})
    ref = conv.render()["post"]
    conv.close()
    e = {k: post_rms(v, ref) for k, v in frames.items()}
    print(f"{name}: post-gamma RMS vs 1024 spp at 16 spp: plain {e['plain']:.5f}, guided {e['guided']:.5f}, "
          f"variance-guided {e['variance']:.5f}; ratio to plain {e['variance'] / e['plain']:.3f}, "
          f"to guided {e['variance'] / e['guided']:.3f}")
    assert e["variance"] < e["plain"]


# ---- the other hosts ------------------------------------------------------------------------------------------
_NODE_SCRIPT = r'''
import fs from 'fs';
import { pathToFileURL } from 'url';
const [root, scenePath, out] = process.argv.slice(2);
(async () => {
const { GpuRayTracer } = await import(pathToFileURL(root + '/blenderraytracer_amd/js/gpu-ray-tracer.mjs').href);
const rt = new GpuRayTracer({ width: 64, height: 48 }, { seed: 3 });
if (!rt.loadFromJSON(JSON.parse(fs.readFileSync(scenePath, 'utf8')))) process.exit(3);
rt.updateRenderSettings({ samples: 8, guidedDenoise: true, guidedVariance: true });
rt.updateRenderSettings({ samples: 8 });                       // without the keys: the filter stays as it was
if (rt.guidedVariance !== true || rt.guidedDenoise !== true) process.exit(4);
const res = await rt.renderBuffers({ batchSamples: 4 });       // guidedVariance implies the estimate
fs.writeFileSync(out + '.rgba8', Buffer.from(res.rgba8.buffer, res.rgba8.byteOffset, res.rgba8.byteLength));
rt.updateRenderSettings({ samples: 8, guidedVariance: false });
const guided = await rt.renderBuffers({ batchSamples: 4 });
fs.writeFileSync(out + '.guided', Buffer.from(guided.rgba8.buffer, guided.rgba8.byteOffset, guided.rgba8.byteLength));
})().catch((e) => { console.error(e); process.exit(1); });
'''


def test_node_variance_guided_frame_equals_pythons(gpu, tmp_path):
    import os
    import shutil
    import subprocess
    from blenderraytracer_amd.scene import scene_path
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "blenderraytracer_amd", "lib", "rt_napi.node")), "rt_napi.node missing"
    script = tmp_path / "vguided.mjs"
    script.write_text(_NODE_SCRIPT)
    out = str(tmp_path / "node")
    r = subprocess.run([node, str(script), root, scene_path("sample_scene.json"), out], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    py = renders("sample_scene")
    assert np.array_equal(np.fromfile(out + ".rgba8", dtype=np.uint8).reshape(48, 64, 4), py["vguided"]["rgba8"])
    assert np.array_equal(np.fromfile(out + ".guided", dtype=np.uint8).reshape(48, 64, 4), py["guided"]["rgba8"])


def test_cli_variance_guided_frame_equals_pythons(gpu, tmp_path):
    import os
    import subprocess
    from blenderraytracer_amd.scene import scene_path
    from test_cli import CLI, read_pam
    assert os.path.exists(CLI), "rt_render_cli missing"
    out = tmp_path / "img.pam"
    args = [CLI, scene_path("sample_scene.json"), "--width", "64", "--height", "48", "--spp", str(SPP), "--seed", "3",
            "--batch", str(BATCH), "--out", str(out)]
    py = renders("sample_scene")
    for extra in (["--guided-variance"], ["--guided-variance", repr(GUIDED_SIGMA_VARIANCE)]):   # implies --guided
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(read_pam(out), py["vguided"]["rgba8"]), extra
    r = subprocess.run(args + ["--guided"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and np.array_equal(read_pam(out), py["guided"]["rgba8"]), r.stderr
    r = subprocess.run(args + ["--guided-variance", "-1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "guided-variance" in r.stderr
