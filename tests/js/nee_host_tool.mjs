// Test driver for the Node host's emitter sampling (called by tests/test_emitters_gpu.py).  TEST INFRASTRUCTURE.
//   node nee_host_tool.mjs render <scene> <w> <h> <seed> <spp> <depth> <out.bin>  -> GPU render with
//       updateRenderSettings({ emitterSampling: true }) in sample order (RGBA8)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { GpuRayTracer } from '../../blenderraytracer_amd/js/gpu-ray-tracer.mjs';

const HERE = path.dirname(fileURLToPath(import.meta.url));
const REPO = path.resolve(HERE, '..', '..');

async function main() {
    const [cmd, scene, w, h, seed, spp, depth, out] = process.argv.slice(2);
    if (cmd !== 'render') throw new Error('unknown command ' + cmd);
    const json = JSON.parse(fs.readFileSync(path.join(REPO, 'scenes', scene + '.json'), 'utf8'));
    const rt = new GpuRayTracer({ width: +w, height: +h }, { seed: +seed, sumOrder: 'sample' });
    if (!rt.loadFromJSON(json)) throw new Error('loadFromJSON failed');
    if (rt.emitterSampling !== false) throw new Error('emitter sampling must be off by default');
    rt.updateRenderSettings({ samples: +spp, maxBounces: +depth, emitterSampling: true });
    if (rt.emitterSampling !== true) throw new Error('updateRenderSettings did not switch emitter sampling on');
    await rt.render();
    fs.writeFileSync(out, Buffer.from(rt.imageData.data.buffer));
}

main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
