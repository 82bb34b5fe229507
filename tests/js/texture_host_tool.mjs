// Test driver for the Node host's texture support (called by tests/test_textures*.py).  TEST INFRASTRUCTURE.
//   node texture_host_tool.mjs pack <scene.json> <w> <h> <seed>  -> JSON: the twin loader's packed scene
//   node texture_host_tool.mjs perms <seed> <k>...                -> JSON: world table + texturePermutation(seed, k)
//   node texture_host_tool.mjs lowering                           -> JSON: SolidColor / base Texture vs plain materials
//   node texture_host_tool.mjs shapes                             -> JSON: reference-shaped (non-twin) objects packed
//   node texture_host_tool.mjs edit                               -> JSON: scene-change detection sees a texture edit
//   node texture_host_tool.mjs render <case> <out.bin>            -> GPU render of a fixture case (RGBA8)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { GpuRayTracer } from '../../blenderraytracer_amd/js/gpu-ray-tracer.mjs';
import { packScene, TEXTURE_BYTES } from '../../blenderraytracer_amd/js/pack.mjs';
import { permutation, texturePermutation } from '../../blenderraytracer_amd/js/keyed-rng.mjs';
import * as M from '../../blenderraytracer_amd/js/scene-model.mjs';

const HERE = path.dirname(fileURLToPath(import.meta.url));
const REPO = path.resolve(HERE, '..', '..');
const b64 = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64');

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
const dump = (p) => ({
    objects: b64(p.objects), materials: b64(p.materials), triangles: b64(p.triangles), perm: Array.from(p.perm),
    textures: decodeTextures(p), materialTexture: Array.from(p.materialTexture), texturePerms: Array.from(p.texturePerms),
});

function world(objs) {
    const w = new M.World(permutation(5));
    objs.forEach((o) => w.add(o));
    return w;
}
const cam = () => new M.Camera(new M.Vec3(3, 2, 2), new M.Vec3(0, 0, -1), new M.Vec3(0, 1, 0), 45, 1.5, 0.0, 10.0);
const V = (x, y, z) => new M.Vec3(x, y, z);

async function main() {
    const [cmd, ...args] = process.argv.slice(2);
    if (cmd === 'pack') {
        const rt = new GpuRayTracer({ width: +args[1], height: +args[2] }, { seed: +args[3] });
        if (!rt.loadFromJSON(JSON.parse(fs.readFileSync(path.join(REPO, 'scenes', args[0]), 'utf8')))) throw new Error('loadFromJSON failed');
        process.stdout.write(JSON.stringify(dump(packScene(rt.world, rt.camera))));
    } else if (cmd === 'perms') {
        const seed = +args[0];
        process.stdout.write(JSON.stringify({ world: permutation(seed), textures: args.slice(1).map((k) => texturePermutation(seed, +k)) }));
    } else if (cmd === 'lowering') {
        const c = V(0.7, 0.3, 0.2);
        const textured = world([new M.Sphere(V(0, 0, -1), 0.5, new M.TexturedLambertian(new M.SolidColor(c))),
                                new M.Sphere(V(1, 0, -1), 0.5, new M.TexturedMetal(new M.SolidColor(c), 0.25)),
                                new M.Sphere(V(2, 0, -1), 0.5, new M.TexturedLambertian({ value() { return V(1, 1, 1); } }))]);
        const plain = world([new M.Sphere(V(0, 0, -1), 0.5, new M.Lambertian(c)), new M.Sphere(V(1, 0, -1), 0.5, new M.Metal(c, 0.25)),
                             new M.Sphere(V(2, 0, -1), 0.5, new M.Lambertian(V(1, 1, 1)))]);
        process.stdout.write(JSON.stringify({ textured: dump(packScene(textured, cam())), plain: dump(packScene(plain, cam())) }));
    } else if (cmd === 'shapes') {
        // objects shaped like the reference's (plain fields, classes of the reference's names defined here, a shared
        // texture, a mesh whose triangles share one textured material)
        class MarbleTexture { constructor(p, scale) { this.scale = scale; this.noise = { p }; } value() {} }
        class WoodTexture { constructor(p, scale) { this.scale = scale; this.noise = { p }; } value() {} }
        const checker = { odd: V(0.1, 0.1, 0.1), even: V(0.9, 0.9, 0.9), scale: 4, value() {} };
        const marble = new MarbleTexture(texturePermutation(3, 0), 2), wood = new WoodTexture(texturePermutation(3, 1), 1);
        const shared = { texture: checker, scatter() {} };
        const meshMat = { texture: wood, roughness: 0.5, scatter() {} };
        const mesh = new M.TriangleMesh([V(0, 0, 0), V(1, 0, 0), V(0, 1, 0), V(1, 1, 0)], [0, 1, 2, 1, 3, 2], meshMat);
        const w = world([new M.Sphere(V(0, 0, -1), 0.5, shared), new M.Sphere(V(1, 0, -1), 0.5, { texture: checker, roughness: 0.1 }),
                         new M.Box(V(-1, -1, -1), V(0, 0, 0), { texture: marble }), mesh, new M.Sphere(V(2, 0, -1), 0.5, shared),
                         new M.Sphere(V(3, 0, -1), 0.5, new M.Dielectric(1.5))]);
        process.stdout.write(JSON.stringify(dump(packScene(w, cam()))));
    } else if (cmd === 'edit') {
        const tex = new M.CheckerTexture(V(0, 0, 0), V(1, 1, 1), 10);
        const w = world([new M.Sphere(V(0, 0, -1), 0.5, new M.TexturedLambertian(tex))]);
        const a = packScene(w, cam());
        tex.scale = 3;
        const b = packScene(w, cam());
        const same = (k) => Buffer.from(a[k].buffer, a[k].byteOffset, a[k].byteLength).equals(Buffer.from(b[k].buffer, b[k].byteOffset, b[k].byteLength));
        process.stdout.write(JSON.stringify({ texturesSame: same('textures'), materialsSame: same('materials') }));
    } else if (cmd === 'render') {
        // case 1 through the twin classes (no JSON): GpuRayTracer's world built by hand like the scene file
        const man = JSON.parse(fs.readFileSync(path.join(REPO, 'tests', 'golden', 'textures', 'manifest.json'), 'utf8'));
        const c = man.cases[args[0]];
        const json = JSON.parse(fs.readFileSync(path.join(REPO, 'scenes', c.scene), 'utf8'));
        const rt = new GpuRayTracer({ width: c.requested[0], height: c.requested[1] }, { seed: c.seed, sumOrder: 'sample' });
        if (!rt.loadFromJSON(json)) throw new Error('loadFromJSON failed');      // camera and plain objects
        const vec = (a) => V(a[0], a[1], a[2]);
        let k = 0;
        rt.world.objects.forEach((o, i) => {                                          // the twin classes, built by hand
            const m = json.objects[i].material, t = m.texture;
            if (!t || (m.type !== 'lambertian' && m.type !== 'metal')) return;
            const color = vec(m.color);
            const tex = t.type === 'checkerboard' ? new M.CheckerTexture(t.odd ? vec(t.odd) : color.mul(0.2), t.even ? vec(t.even) : color, t.scale !== undefined ? t.scale : 10)
                : t.type === 'noise' ? new M.NoiseTexture(texturePermutation(c.seed, k++), t.scale !== undefined ? t.scale : 1)
                : t.type === 'marble' ? new M.MarbleTexture(texturePermutation(c.seed, k++), t.scale !== undefined ? t.scale : 1)
                : new M.WoodTexture(texturePermutation(c.seed, k++), t.scale !== undefined ? t.scale : 1);
            o.material = m.type === 'metal' ? new M.TexturedMetal(tex, m.roughness) : new M.TexturedLambertian(tex);
        });
        rt.updateRenderSettings(c.settings_in);
        await rt.render();
        fs.writeFileSync(args[1], Buffer.from(rt.imageData.data.buffer));
    } else {
        throw new Error('unknown command ' + cmd);
    }
}

main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
