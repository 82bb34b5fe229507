// Golden-vector generator for procedural textures: runs the REAL reference renderer (its own
// TexturedLambertian / TexturedMetal and texture classes) under Node with Math.random replaced by the keyed
// RNG, and writes tests/golden/textures/ (its own manifest.json, kats.json.gz).  TEST INFRASTRUCTURE ONLY:
// runs where the reference checkout is (RT_REFERENCE), never on the GPU box, never imported by product code;
// none of the reference's text is copied into the repository (it is imported from a temp copy at run time,
// like oracle/ref_harness/run_reference.mjs).
//
// The reference's scene loader ignores the "texture" extension of scenes/tex_*.json (INTEGRATION.md), so
// each case is loaded through the reference's own loadFromJSON and then every flagged object's material (and
// every triangle's, for a mesh) is replaced by the reference's textured material built from the reference's
// texture classes, the keyed stream select(0xFFFFFFFD, k) chosen before the k-th noise-bearing texture is
// constructed (its PerlinNoise shuffles with Math.random), k in World.objects order.
//
// Range condition: while rendering (and for the KATs) Math.sin and PerlinNoise.prototype.noise are wrapped;
// the run fails unless every |sin argument| <= 2^19 pi/2 and every |noise coordinate| < 2^31, the range in
// which the project's V8 sin (js_math.h) and integer lattice are exact.  The maxima go into the manifest.
//
// usage: node tests/js/texture_reference.mjs [--only name,name] [--kats]
import fs from 'fs';
import os from 'os';
import path from 'path';
import zlib from 'zlib';
import { fileURLToPath, pathToFileURL } from 'url';
import { KeyedStream, permutation, texturePermutation } from '../../blenderraytracer_amd/js/keyed-rng.mjs';
import { packScene, TEXTURE_BYTES } from '../../blenderraytracer_amd/js/pack.mjs';

const HERE = path.dirname(fileURLToPath(import.meta.url));
const REPO = path.resolve(HERE, '..', '..');
const REF = process.env.RT_REFERENCE || '/root/reference';
const OUT = path.join(REPO, 'tests', 'golden', 'textures');

const CASES = [
    { name: 'tex_checker_spheres', scene: 'tex_checker_spheres.json', width: 64, height: 48, seed: 11,
      settings: { maxBounces: 5, samples: 16 }, crop: null },
    { name: 'tex_kitchen_sink', scene: 'tex_kitchen_sink.json', width: 48, height: 32, seed: 12,
      settings: { maxBounces: 5, samples: 8, antiAliasing: 'stochastic' }, crop: null },
    { name: 'tex_mesh_wood_crop', scene: 'tex_mesh_wood_crop.json', width: 64, height: 48, seed: 13,
      settings: { maxBounces: 8, samples: 32 }, crop: [21, 17, 20, 12] },
];

const SIN_LIMIT = 524288 * Math.PI / 2, NOISE_LIMIT = 2147483648;

function prepareReference() {
    const dir = fs.mkdtempSync(path.join(os.tmpdir(), 'rt-ref-'));
    fs.mkdirSync(path.join(dir, 'js'));
    for (const f of fs.readdirSync(path.join(REF, 'js'))) {
        let src = fs.readFileSync(path.join(REF, 'js', f), 'utf8');
        // optional chaining does not parse on Node 12 (updateCamera, off the render path)
        if (f === 'ray-tracer.js') src = src.replace(/this\.camera\?\.([A-Za-z]+)/g, '(this.camera && this.camera.$1)');
        fs.writeFileSync(path.join(dir, 'js', f), src);
    }
    fs.writeFileSync(path.join(dir, 'package.json'), '{"type":"module"}');
    return dir;
}

global.window = { renderCancelled: false };
global.performance = { now: () => Date.now() };
const realLog = console.log;
console.log = () => {};
console.warn = () => {};
console.error = () => {};

function makeCanvas(w, h) {
    return {
        width: w, height: h, style: {},
        getContext: () => ({
            createImageData: (cw, ch) => ({ width: cw, height: ch, data: new Uint8ClampedArray(cw * ch * 4) }),
            putImageData() {},
        }),
    };
}

let stream = new KeyedStream(0);
let drawCounter = null;
let curPix = -1;
Math.random = () => { if (drawCounter && curPix >= 0) drawCounter[curPix]++; return stream.next(); };

// range recording
const range = { sin: 0, noise: 0, on: false };
const realSin = Math.sin;
Math.sin = (x) => { if (range.on && Math.abs(x) > range.sin) range.sin = Math.abs(x); return realSin(x); };
function wrapNoise(PerlinNoise) {
    const orig = PerlinNoise.prototype.noise;
    PerlinNoise.prototype.noise = function noise(p) {
        if (range.on) range.noise = Math.max(range.noise, Math.abs(p.x), Math.abs(p.y), Math.abs(p.z));
        return orig.call(this, p);
    };
}
function startRange() { range.sin = 0; range.noise = 0; range.on = true; }
function endRange(what) {
    range.on = false;
    if (!(range.sin <= SIN_LIMIT) || !(range.noise < NOISE_LIMIT))
        throw new Error(`${what}: outside the exact range: max |sin argument| ${range.sin}, max |noise coordinate| ${range.noise}`);
    return { max_sin_argument: range.sin, max_noise_coordinate: range.noise };
}

function enc(v) {
    if (typeof v === 'number') {
        if (Number.isNaN(v)) return 'NaN';
        if (v === Infinity) return 'Infinity';
        if (v === -Infinity) return '-Infinity';
        return v;
    }
    if (Array.isArray(v)) return v.map(enc);
    if (v && typeof v === 'object') { const o = {}; for (const k of Object.keys(v)) o[k] = enc(v[k]); return o; }
    return v;
}
const v3 = (v) => [v.x, v.y, v.z];

function loadScene(name) { return JSON.parse(fs.readFileSync(path.join(REPO, 'scenes', name), 'utf8')); }
function writeGz(file, typed) {
    fs.writeFileSync(path.join(OUT, file), zlib.gzipSync(Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength), { level: 9 }));
}

// The reference's textured material for a JSON material with the "texture" extension, or null (plain).
// nextK: { k } counts the noise-bearing textures; seed: the render seed of the keyed streams.
function texturedMaterial(mods, m, nextK) {
    const { Vec3, CheckerTexture, NoiseTexture, MarbleTexture, WoodTexture, TexturedLambertian, TexturedMetal } = mods;
    if (!m || typeof m.type !== 'string') return null;
    const mt = m.type.toLowerCase();
    if (mt !== 'lambertian' && mt !== 'metal') return null;
    const t = m.texture;
    if (!t || typeof t !== 'object' || Array.isArray(t)) return null;
    const vec = (a) => (Array.isArray(a) && a.length >= 3 ? new Vec3(a[0], a[1], a[2]) : new Vec3(0, 0, 0));
    const color = vec(m.color);
    const scale = (d) => (t.scale !== undefined ? t.scale : d);
    const noisy = (Cls) => { stream.select(0xFFFFFFFD, nextK.k++); return new Cls(scale(1)); };
    let tex;
    switch (t.type) {
        case 'checkerboard':
            tex = new CheckerTexture(t.odd !== undefined ? vec(t.odd) : color.mul(0.2), t.even !== undefined ? vec(t.even) : color, scale(10));
            break;
        case 'noise': tex = noisy(NoiseTexture); break;
        case 'marble': tex = noisy(MarbleTexture); break;
        case 'wood': tex = noisy(WoodTexture); break;
        default: return null;
    }
    return mt === 'metal' ? new TexturedMetal(tex, m.roughness !== undefined ? m.roughness : 0.0) : new TexturedLambertian(tex);
}

// JSON objects the reference's loader turned into World objects (scene-loader.js:90-137), in order
function acceptedObjects(json) {
    const kinds = ['sphere', 'plane', 'box', 'triangle', 'mesh'];
    return (json.objects || []).filter((o) => o && o.type && kinds.includes(String(o.type).toLowerCase()) &&
        (String(o.type).toLowerCase() !== 'mesh' || (o.vertices && o.indices)));
}

function decodeTextures(p) {
    const n = p.textures.byteLength / TEXTURE_BYTES;
    const buf = p.textures.buffer.slice(p.textures.byteOffset, p.textures.byteOffset + p.textures.byteLength);
    const ti = new Int32Array(buf), tf = new Float64Array(buf);
    const out = [];
    for (let i = 0; i < n; i++) {
        const b = i * (TEXTURE_BYTES / 8);
        out.push({ type: ti[2 * b], perm: ti[2 * b + 1], scale: tf[b + 1], odd: Array.from(tf.subarray(b + 2, b + 5)), even: Array.from(tf.subarray(b + 5, b + 8)) });
    }
    return out;
}

async function runCase(mods, c) {
    const { RayTracer, Vec3 } = mods;
    const canvas = makeCanvas(c.width, c.height);
    stream = new KeyedStream(c.seed);
    stream.select(0xFFFFFFFE, 0xFFFFFFFE);           // constructor's default scene: irrelevant stream
    const rt = new RayTracer(canvas);
    stream.select(0xFFFFFFFF, 0xFFFFFFFF);           // PERM stream for the loaded World's PerlinNoise
    const json = loadScene(c.scene);
    if (!rt.loadFromJSON(JSON.parse(JSON.stringify(json)))) throw new Error('loadFromJSON failed for ' + c.name);
    rt.updateRenderSettings(c.settings);
    const permExpect = permutation(c.seed);
    if (rt.world.cloudNoise.p.some((x, i) => x !== permExpect[i])) throw new Error('perm stream mismatch');
    // the textured materials, built from the reference's own classes
    const acc = acceptedObjects(json);
    if (acc.length !== rt.world.objects.length) throw new Error(`${c.name}: ${acc.length} JSON objects for ${rt.world.objects.length} World objects`);
    const nextK = { k: 0 };
    let textured = 0;
    acc.forEach((o, i) => {
        const mat = texturedMaterial(mods, o.material, nextK);
        if (!mat) return;
        textured++;
        const obj = rt.world.objects[i];
        obj.material = mat;
        if (obj.triangles) for (const t of obj.triangles) t.material = mat;
    });
    const W = rt.width, H = rt.height;
    const [x0, y0, cw, ch] = c.crop || [0, 0, W, H];
    const n = cw * ch;
    const linear = new Float64Array(n * 3), post = new Float64Array(n * 3);
    const rgba = new Uint8Array(n * 4);
    const segs = new Uint32Array(n), draws = new Uint32Array(n);
    const fullSegs = new Uint32Array(W * H), fullDraws = new Uint32Array(W * H);
    drawCounter = fullDraws;
    const localIndex = (p) => { const row = Math.floor(p / W), col = p % W; return (row - y0) * cw + (col - x0); };
    const origAA = rt.getAntiAliasSample.bind(rt);
    rt.getAntiAliasSample = (i, j, s) => {
        curPix = (H - 1 - j) * W + i;
        stream.select(curPix, s);
        return origAA(i, j, s);
    };
    const origTM = rt.toneMap.bind(rt);
    rt.toneMap = (color) => { linear.set(v3(color), localIndex(curPix) * 3); return origTM(color); };
    const origGC = rt.gammaCorrect.bind(rt);
    rt.gammaCorrect = (color) => { const r = origGC(color); post.set(v3(r), localIndex(curPix) * 3); return r; };
    const world = rt.world;
    const origHit = world.hit.bind(world);
    world.hit = (ray, a, b) => { fullSegs[curPix]++; return origHit(ray, a, b); };
    const sampleCount = rt.antiAliasing === 'none' ? 1 : rt.samples;
    startRange();
    const t0 = process.hrtime.bigint();
    if (!c.crop) {
        await rt.render();
        rgba.set(rt.imageData.data);
    } else {
        // the loop body of RayTracer.render (ray-tracer.js:189-252), restricted to the crop's rows / columns
        const tmp = new Uint8ClampedArray(4);
        for (let j = H - 1; j >= 0; j--) {
            const row = H - 1 - j;
            if (row < y0 || row >= y0 + ch) continue;
            for (let i = x0; i < x0 + cw; i++) {
                let color = new Vec3(0, 0, 0);
                for (let s = 0; s < sampleCount; s++) {
                    const sm = rt.getAntiAliasSample(i, j, s);
                    color = color.add(rt.rayColor(rt.camera.getRay(sm.u, sm.v), rt.maxBounces));
                }
                color = rt.gammaCorrect(rt.toneMap(color.div(sampleCount)));
                tmp[0] = Math.min(255, Math.max(0, Math.floor(color.x * 255)));
                tmp[1] = Math.min(255, Math.max(0, Math.floor(color.y * 255)));
                tmp[2] = Math.min(255, Math.max(0, Math.floor(color.z * 255)));
                tmp[3] = 255;
                rgba.set(tmp, ((row - y0) * cw + (i - x0)) * 4);
            }
        }
    }
    const secs = Number(process.hrtime.bigint() - t0) / 1e9;
    const rng = endRange(c.name);
    drawCounter = null; curPix = -1;
    for (let r = 0; r < ch; r++) for (let x = 0; x < cw; x++) {
        const p = (y0 + r) * W + (x0 + x);
        segs[r * cw + x] = fullSegs[p]; draws[r * cw + x] = fullDraws[p];
    }
    world.hit = origHit;
    // what the drop-in's packer makes of these real reference objects
    const packed = packScene(rt.world, rt.camera);
    const files = {};
    for (const [k, arr] of Object.entries({ linear, post, rgba8: rgba, segs, draws })) {
        files[k] = `${c.name}.${k}.gz`;
        writeGz(files[k], arr);
    }
    return {
        name: c.name, scene: c.scene, seed: c.seed, requested: [c.width, c.height], width: W, height: H,
        crop: [x0, y0, cw, ch], settings_in: c.settings, background_in: null,
        resolved: { maxBounces: rt.maxBounces, samples: rt.samples, gamma: rt.gamma, exposure: rt.exposure,
                    toneMapping: rt.toneMapping, antiAliasing: rt.antiAliasing, skyIntensity: rt.world.skyIntensity },
        textured_objects: textured,
        packed: { textures: decodeTextures(packed), materialTexture: Array.from(packed.materialTexture),
                  texturePerms: Array.from(packed.texturePerms), numMaterials: packed.materials.byteLength / 72 },
        range: rng, files, js_seconds: secs, js_samples: n * sampleCount,
    };
}

// ---- known-answer vectors: texture values and textured scatters -----------------------------------
function kats(mods) {
    const { Vec3, Ray, HitRecord, CheckerTexture, NoiseTexture, MarbleTexture, WoodTexture, SolidColor,
            TexturedLambertian, TexturedMetal } = mods;
    const SEED = 77;
    const gen = new KeyedStream(515151);
    let gk = 0;
    const U = (a, b) => { gen.select(9, gk++); return a + (b - a) * gen.next(); };
    stream = new KeyedStream(SEED);
    let k = 0;
    const noisy = (Cls, scale) => { stream.select(0xFFFFFFFD, k); const t = new Cls(scale); t.__k = k++; return t; };
    // reach: the largest |coordinate x scale| probed (inside the exact range of every sin / noise argument)
    const specs = [
        { type: 'checker', scale: 10, reach: 5e5, make: (s) => new CheckerTexture(new Vec3(0.1, 0.2, 0.3), new Vec3(0.9, 0.8, 0.7), s) },
        { type: 'checker', scale: 0.75, reach: 5e5, make: (s) => new CheckerTexture(new Vec3(0, 0, 0), new Vec3(1, 1, 1), s) },
        { type: 'noise', scale: 1, reach: 2e9, make: (s) => noisy(NoiseTexture, s) },
        { type: 'noise', scale: 6, reach: 2e9, make: (s) => noisy(NoiseTexture, s) },
        { type: 'marble', scale: 1, reach: 4e5, make: (s) => noisy(MarbleTexture, s) },
        { type: 'marble', scale: 2.5, reach: 4e5, make: (s) => noisy(MarbleTexture, s) },
        { type: 'wood', scale: 1, reach: 4e5, make: (s) => noisy(WoodTexture, s) },
        { type: 'wood', scale: 1.5, reach: 4e5, make: (s) => noisy(WoodTexture, s) },
    ];
    const out = { seed: SEED, textures: [], scatter: [] };
    startRange();
    const texObjs = [];
    for (const sp of specs) {
        const tex = sp.make(sp.scale);
        texObjs.push(tex);
        const pts = [];
        for (let q = 0; q < 60; q++) pts.push([U(-3, 3), U(-3, 3), U(-3, 3)]);                    // around the origin, both signs
        for (let q = 0; q < 30; q++) pts.push([U(-40, 40), U(-40, 40), U(-40, 40)]);
        for (let q = 0; q < 20; q++) pts.push([U(-1e3, 1e3), U(-1e3, 1e3), U(-1e3, 1e3)]);
        // lattice edges: exact integers and half-integers in p * scale where scale is exact, and in p
        for (const a of [0, 1, -1, 2, -3, 0.5, -0.5, 1.5, -2.5, 255, 256, -256, 257.5]) {
            pts.push([a, 0.25, -0.75], [0.3, a, a], [a, a, a], [a / sp.scale, a / sp.scale, a / sp.scale]);
        }
        pts.push([0, 0, 0]);
        // within 1e-12 of a checker boundary (scale * x = k pi) and of a lattice plane
        for (const kk of [1, -1, 2, 7, -12]) for (const e of [-1e-12, 0, 1e-12, -1e-15, 1e-15]) {
            pts.push([kk * Math.PI / sp.scale + e, 0.37, -1.21], [0.61, kk * Math.PI / sp.scale + e, 0.45], [kk / sp.scale + e, 0.5, 0.5]);
        }
        // magnitudes up to the range limit
        for (const f of [0.01, 0.1, 0.5, 0.99]) for (let q = 0; q < 3; q++) {
            const r = f * sp.reach / sp.scale;
            pts.push([U(-r, r), U(-r, r), U(-r, r)], [r, -r, r], [-r, r * 0.5, -r]);
        }
        const values = pts.map((p) => v3(tex.value(0, 0, new Vec3(p[0], p[1], p[2]))));
        out.textures.push({ type: sp.type, scale: sp.scale, odd: tex.odd ? v3(tex.odd) : null, even: tex.even ? v3(tex.even) : null,
                            k: tex.__k !== undefined ? tex.__k : -1, perm: tex.noise ? tex.noise.p.slice() : null, points: pts, values });
    }
    // TexturedLambertian / TexturedMetal scatter (layout of tests/golden/kats.json.gz "scatter"): the stream
    // is the render stream of (pixel, sample) under SEED
    const randVec = (a, b) => new Vec3(U(a, b), U(a, b), U(a, b));
    const mats = [];
    texObjs.forEach((tex, ti) => {
        mats.push({ m: { type: 'lambertian', texture: ti }, make: () => new TexturedLambertian(tex) });
        mats.push({ m: { type: 'metal', roughness: 0.35, texture: ti }, make: () => new TexturedMetal(tex, 0.35) });
    });
    mats.push({ m: { type: 'metal', roughness: 1, texture: 0 }, make: () => new TexturedMetal(texObjs[0], 2.5) });
    mats.push({ m: { type: 'lambertian', solid: [0.7, 0.3, 0.2] }, make: () => new TexturedLambertian(new SolidColor(new Vec3(0.7, 0.3, 0.2))) });
    mats.push({ m: { type: 'metal', roughness: 0.2, solid: [0.8, 0.6, 0.2] }, make: () => new TexturedMetal(new SolidColor(new Vec3(0.8, 0.6, 0.2)), 0.2) });
    for (const mm of mats) {
        const mat = mm.make();
        for (let q = 0; q < 24; q++) {
            const d = randVec(-1, 1).mul(U(0.3, 2));
            const nrm = randVec(-1, 1).normalize();
            const rec = new HitRecord();
            rec.t = U(0.1, 3); rec.point = randVec(-4, 4);
            rec.setFaceNormal(new Ray(new Vec3(0, 0, 0), d), nrm);
            stream.select(2000 + q, 55);
            const before = stream.k;
            const sr = mat.scatter(new Ray(new Vec3(0, 0, 0), d), rec);
            out.scatter.push({
                material: mm.m, d: v3(d), point: v3(rec.point), normal: v3(rec.normal), frontFace: rec.frontFace,
                seed: SEED, pixel: 2000 + q, sample: 55, draws: stream.k - before,
                result: sr ? { origin: v3(sr.scattered.origin), dir: v3(sr.scattered.direction), attenuation: v3(sr.attenuation) } : null,
                emitted: v3(mat.emitted(0, 0, rec.point)),
            });
        }
    }
    out.range = endRange('kats');
    // the keyed permutations the three hosts must derive for these textures
    for (const t of out.textures) if (t.perm) {
        const e = texturePermutation(SEED, t.k);
        if (t.perm.some((x, i) => x !== e[i])) throw new Error('texturePermutation mismatch with the reference shuffle');
    }
    return out;
}

async function main() {
    const argv = process.argv.slice(2);
    const only = argv.includes('--only') ? argv[argv.indexOf('--only') + 1].split(',') : null;
    const dir = prepareReference();
    const url = (f) => pathToFileURL(path.join(dir, 'js', f)).href;
    const mods = {
        ...(await import(url('ray-tracer.js'))), ...(await import(url('math.js'))), ...(await import(url('geometry.js'))),
        ...(await import(url('materials.js'))), ...(await import(url('camera.js'))), ...(await import(url('world.js'))),
        ...(await import(url('textures.js'))), ...(await import(url('noise.js'))),
    };
    wrapNoise(mods.PerlinNoise);
    fs.mkdirSync(OUT, { recursive: true });
    const manifestPath = path.join(OUT, 'manifest.json');
    const manifest = fs.existsSync(manifestPath) ? JSON.parse(fs.readFileSync(manifestPath, 'utf8')) : { cases: {} };
    manifest.generator = 'tests/js/texture_reference.mjs';
    manifest.node = process.version;
    manifest.limits = { max_sin_argument: SIN_LIMIT, max_noise_coordinate: NOISE_LIMIT };
    for (const c of CASES) {
        if (only && !only.includes(c.name)) continue;
        const rec = await runCase(mods, c);
        manifest.cases[c.name] = enc(rec);
        realLog(`${c.name}: ${rec.width}x${rec.height} crop ${rec.crop} ${rec.js_samples} samples in ${rec.js_seconds.toFixed(2)} s, ` +
                `${rec.textured_objects} textured objects, max |sin arg| ${rec.range.max_sin_argument.toPrecision(4)}, max |noise coord| ${rec.range.max_noise_coordinate.toPrecision(4)}`);
    }
    if (!only || argv.includes('--kats')) {
        const k = kats(mods);
        fs.writeFileSync(path.join(OUT, 'kats.json.gz'), zlib.gzipSync(JSON.stringify(enc(k)), { level: 9 }));
        manifest.kats_range = k.range;
        realLog(`kats: ${k.textures.length} textures x ${k.textures[0].points.length} points, ${k.scatter.length} scatters, ` +
                `max |sin arg| ${k.range.max_sin_argument.toPrecision(6)}, max |noise coord| ${k.range.max_noise_coordinate.toPrecision(6)}`);
    }
    fs.writeFileSync(manifestPath, JSON.stringify(manifest, null, 1) + '\n');
    fs.rmdirSync(dir, { recursive: true });
}

main().catch((e) => { realLog(e && e.stack || e); process.exit(1); });
