// Test driver for the Node host's direct-lighting support (called by tests/test_lights*.py).  TEST INFRASTRUCTURE.
//   node lights_host_tool.mjs pack <scene.json path> <w> <h> <seed>  -> JSON: the twin loader's scene packed without
//                                                                       and with { lights: true }
//   node lights_host_tool.mjs shapes                                  -> JSON: reference-shaped (non-twin) light objects packed
//   node lights_host_tool.mjs render <case> <out.bin>                 -> GPU render of a fixture case (RGBA8)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { GpuRayTracer } from '../../blenderraytracer_amd/js/gpu-ray-tracer.mjs';
import { packScene, LIGHT_BYTES } from '../../blenderraytracer_amd/js/pack.mjs';
import { permutation } from '../../blenderraytracer_amd/js/keyed-rng.mjs';
import * as M from '../../blenderraytracer_amd/js/scene-model.mjs';

const HERE = path.dirname(fileURLToPath(import.meta.url));
const REPO = path.resolve(HERE, '..', '..');
const b64 = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64');
const V = (x, y, z) => new M.Vec3(x, y, z);

// every field of a packed scene, typed arrays as base64
function dump(p) {
    const o = {};
    for (const k of Object.keys(p)) o[k] = ArrayBuffer.isView(p[k]) ? b64(p[k]) : p[k];
    return o;
}

function caseJson(name) {
    const man = JSON.parse(fs.readFileSync(path.join(REPO, 'tests', 'golden', 'lights', 'manifest.json'), 'utf8'));
    const c = man.cases[name];
    const json = JSON.parse(fs.readFileSync(path.join(REPO, 'scenes', c.scene), 'utf8'));
    if (c.lights_in) json.lights = c.lights_in;
    return { c, json };
}

async function main() {
    const [cmd, ...args] = process.argv.slice(2);
    if (cmd === 'pack') {
        const rt = new GpuRayTracer({ width: +args[1], height: +args[2] }, { seed: +args[3] });
        if (!rt.loadFromJSON(JSON.parse(fs.readFileSync(args[0], 'utf8')))) throw new Error('loadFromJSON failed');
        const lit = packScene(rt.world, rt.camera, { lights: true });
        process.stdout.write(JSON.stringify({ unlit: dump(packScene(rt.world, rt.camera)), lit: dump(lit),
                                              lightBytes: LIGHT_BYTES, numLights: rt.world.lights.length }));
    } else if (cmd === 'shapes') {
        // lights shaped like the reference's (lights.js): a PointLight has position / color / intensity, a
        // DirectionalLight also a (normalized) direction and the base class's position (0, 0, 0)
        const w = new M.World(permutation(5));
        w.add(new M.Sphere(V(0, 0, -1), 0.5, new M.Lambertian(V(0.5, 0.5, 0.5))));
        w.lights.push({ position: V(1, 2, 3), color: V(1, 0.5, 0.25), intensity: 8, illuminate() {} });
        w.lights.push({ position: V(0, 0, 0), color: V(0.9, 0.8, 0.7), intensity: 2, direction: V(0, -0.6, 0.8), illuminate() {} });
        const cam = new M.Camera(V(3, 2, 2), V(0, 0, -1), V(0, 1, 0), 45, 1.5, 0.0, 10.0);
        process.stdout.write(JSON.stringify({ lit: dump(packScene(w, cam, { lights: true })), unlit: dump(packScene(w, cam)) }));
    } else if (cmd === 'render') {
        const { c, json } = caseJson(args[0]);
        const rt = new GpuRayTracer({ width: c.requested[0], height: c.requested[1] }, { seed: c.seed, sumOrder: 'sample' });
        if (!rt.loadFromJSON(json)) throw new Error('loadFromJSON failed');
        rt.updateRenderSettings({ ...c.settings_in, directLighting: true });
        await rt.render();
        fs.writeFileSync(args[1], Buffer.from(rt.imageData.data.buffer));
    } else {
        throw new Error('unknown command ' + cmd);
    }
}

main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
