"""Independent reference and inputs for the sphere walks (tests/test_sphere_walks.py, test_sphere_walks_gpu.py).
Plain NumPy binary64; imports nothing of the project, so a hit query is compared with a restatement of the
reference's World.hit and never with another of the project's walks.  TEST INFRASTRUCTURE ONLY.

world_hit / occluded   the reference's closest hit and INTEGRATION.md §8's occlusion rule
FAMILIES, scene(name)  seeded sphere-only scenes in the scene-JSON format, each built to fix one scale-dependent
                       part of build_grid or of a walk to another value than RTOW does
RAY_CLASSES, rays(...) seeded stress rays per scene: the direction and origin patterns that bvh_rays never makes
"""
import numpy as np

INF = float("inf")


# ---- the reference ---------------------------------------------------------------------------------------
def spheres_of(data):
    """(centers n x 3, radii n) of a scene dict's spheres, in World order"""
    objs = data["objects"]
    assert all(o["type"] == "sphere" for o in objs)
    return (np.array([o["center"] for o in objs], dtype=np.float64), np.array([o["radius"] for o in objs], dtype=np.float64))


def world_hit(centers, radii, rays, tmin=0.001, tmax=INF):
    """world.js World.hit over geometry.js Sphere.hit: (t, index) of n x 6 rays (origin, direction); t = +inf and
    index = -1 on a miss.  tmax: a number or one per ray.  Spheres in World order, each tested against the
    running closestT; dots summed x, y, z left to right with separately rounded products (NumPy never fuses)."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    ox, oy, oz, dx, dy, dz = (np.ascontiguousarray(rays[:, k]) for k in range(6))
    n = len(rays)
    closest = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,)).copy()
    best_t = np.full(n, INF)
    best_i = np.full(n, -1, dtype=np.int64)
    a = dx * dx + dy * dy + dz * dz
    with np.errstate(all="ignore"):
        for i in range(len(radii)):
            cx, cy, cz = centers[i]
            r = radii[i]
            ocx, ocy, ocz = ox - cx, oy - cy, oz - cz
            half_b = ocx * dx + ocy * dy + ocz * dz
            c = (ocx * ocx + ocy * ocy + ocz * ocz) - r * r
            disc = half_b * half_b - a * c
            sqrtd = np.sqrt(disc)
            root = (-half_b - sqrtd) / a
            out = (root < tmin) | (closest < root)
            root = np.where(out, (-half_b + sqrtd) / a, root)
            out = (root < tmin) | (closest < root)
            take = ~(disc < 0) & ~out & (root < closest)       # NaN roots fail the last comparison, as in JS
            closest = np.where(take, root, closest)
            best_t = np.where(take, root, best_t)
            best_i = np.where(take, i, best_i)
    return best_t, best_i


def occluded(centers, radii, rays, tmax, tmin=0.001):
    """a shadow ray is occluded iff World.hit(ray, tMin, inf) returns a hit with t < tmax"""
    t, _ = world_hit(centers, radii, rays, tmin)
    return t < np.asarray(tmax, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- scene families --------------------------------------------------------------------------------------
FAMILIES = ("cloud", "offset", "tiny", "flat", "lattice", "clump", "many", "far", "hollow")
OFFSET = np.array([1000.0, 2000.0, -3000.0])


def _material(rng):
    k = int(rng.integers(0, 10))
    if k < 5:
        return {"type": "lambertian", "color": [float(x) for x in rng.uniform(0.1, 0.9, 3)]}
    if k < 8:
        return {"type": "metal", "color": [float(x) for x in rng.uniform(0.4, 1.0, 3)], "roughness": float(rng.uniform(0, 0.5))}
    return {"type": "dielectric", "ior": 1.5}


def _scene(name, centers, radii, mats, cam_from, cam_at, fov=40.0, aperture=0.0):
    objs = [{"type": "sphere", "center": [float(x) for x in c], "radius": float(r), "material": m}
            for c, r, m in zip(centers, radii, mats)]
    cam = {"position": [float(x) for x in cam_from], "lookAt": [float(x) for x in cam_at], "up": [0, 1, 0], "fov": fov,
           "aperture": aperture, "type": "perspective"}
    return {"name": "sphere walks: " + name, "objects": objs, "lights": [], "camera": cam,
            "background": {"type": "gradient", "intensity": 1.0}}


def _cloud(rng, n, half, r0, r1):
    c = rng.uniform(-half, half, (n, 3))
    r = rng.uniform(r0, r1, n)
    return c, r, [_material(rng) for _ in range(n)]


def scene(name):
    """The family's scene dict (always the same: each family has its own fixed seed)."""
    rng = np.random.default_rng(1000 + FAMILIES.index(name))
    if name in ("cloud", "offset", "tiny"):
        c, r, m = _cloud(np.random.default_rng(1000), 300, 5.0, 0.1, 0.5)        # the same cloud in all three
        eye, at = np.array([2.0, 3.0, 16.0]), np.zeros(3)
        if name == "offset":                           # B >> E: margin, pad and grid_far scale with B
            c, eye, at = c + OFFSET, eye + OFFSET, at + OFFSET
        if name == "tiny":                             # hit queries only: tMin = 0.001 swallows a render
            c, r, eye = c * 1e-3, r * 1e-3, eye * 1e-3
        return _scene(name, c, r, m, eye, at, aperture=0.05 if name == "cloud" else 0.0)
    if name == "flat":                                 # 10 x 1 x 10 cells; the walk choice takes the grid
        g = (np.arange(20) - 9.5) * 0.5
        c = np.array([[x, 0.0, z] for z in g for x in g])
        return _scene(name, c, np.full(400, 0.2), [_material(rng) for _ in range(400)], [3.0, 6.0, 11.0], [0, 0, 0])
    if name == "lattice":                              # integer coordinates, the camera on an axis
        g = np.arange(-3, 4, dtype=np.float64)
        c = np.array([[x, y, z] for z in g for y in g for x in g])
        return _scene(name, c, np.full(343, 0.25), [_material(rng) for _ in range(343)], [0.0, 0.0, 14.0], [0, 0, 0])
    if name == "clump":                                # 60 records in one cell: the compaction loop's second pass
        c = np.concatenate([rng.normal(0.0, 0.05, (60, 3)), rng.uniform(-6, 6, (200, 3))])
        r = np.concatenate([np.full(60, 0.3), np.full(200, 0.1)])
        return _scene(name, c, r, [_material(rng) for _ in range(260)], [1.0, 2.0, 9.0], [0, 0, 0], fov=30.0)
    if name == "many":                                 # neither the grid nor the sphere tree fits LDS
        c, r, m = _cloud(rng, 6000, 20.0, 0.1, 0.5)
        return _scene(name, c, r, m, [5.0, 8.0, 60.0], [0, 0, 0])
    if name == "far":                                  # the camera beyond grid_far: the far-origin sweep
        c, r, m = _cloud(rng, 100, 1.0, 0.05, 0.2)
        return _scene(name, c, r, m, [0.0, 0.0, 400.0], [0, 0, 0], fov=0.5)
    if name == "hollow":                               # shells r / -0.9 r; a third coincident sphere on 30 %
        cs, rs, ms = [], [], []
        for _ in range(100):
            c, r = rng.uniform(-5, 5, 3), float(rng.uniform(0.3, 0.8))
            cs += [c, c]
            rs += [r, -0.9 * r]
            ms += [{"type": "dielectric", "ior": 1.5}] * 2
            if rng.uniform() < 0.3:
                cs.append(c)
                rs.append(r)
                ms.append(_material(rng))
        return _scene(name, np.array(cs), np.array(rs), ms, [2.0, 3.0, 16.0], [0, 0, 0])
    raise KeyError(name)


# ---- ray classes -----------------------------------------------------------------------------------------
RAY_CLASSES = ("axis", "zero", "far", "surface", "plane", "scaled")
AXIS_OFFSETS = (0.0, 0.5, 1 - 1e-9, 1.0, 1 + 1e-9)                  # x |r| from the centre
ZERO_VALUES = (0.0, -0.0, 2.0 ** -140, 2.0 ** -120, 2.0 ** -100)    # the replaced direction component
ZERO_ORIGINS = (0.5, 3.9, 4.1, 300.0, 1e4)                          # |origin| on that axis: 2^126 |o| overflows from 4
# A magnitude is used where a sphere cuts that plane, else the ray goes through the picked sphere at its own
# coordinate: 0.5 .. 4.1 occur in the families around the origin, 300 on RTOW alone (its ground), 1e4 in no scene;
# `offset` puts 1000 .. 3000 on the zeroed axis of every ray.
FAR_FACTORS = (32.0, 60.0, 64.0, 65.0, 100.0, 1e4)                  # x (B + E): grid_far = 64 (B + E)
DIR_SCALES = (1e-30, 1e-12, 1e12, 1e25)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def scene_scale(radii):
    """direction lengths are drawn around this, so that t stays well above tMin in the small family too"""
    return float(np.median(np.abs(radii))) / 0.3


def rays(cls, centers, radii, n, seed, grid=None):
    """n seeded rays (n x 6) of a class, with a column of labels (the class's sub-case per ray, for the
    binary32 subset: the offset index of `axis` and `zero` rays).  grid: dict(lo, cs, n, far) of the scene's
    uniform grid (tests/hostcheck_binding.py grid_geometry) for the classes that straddle its constants."""
    rng = np.random.default_rng(seed + 7919 * RAY_CLASSES.index(cls))
    ns = len(radii)
    ar = np.abs(radii)
    S = scene_scale(radii)
    lo, hi = (centers - ar[:, None]).min(0), (centers + ar[:, None]).max(0)
    ext = float((hi - lo).max())
    out = np.zeros((n, 6))
    label = np.zeros(n, dtype=np.int64)
    pick = rng.integers(0, ns, n)
    dlen = S * 10.0 ** rng.uniform(-1, 1, n)
    if cls == "axis":
        dlen = S * 10.0 ** rng.uniform(-2, 2, n)
        for q in range(n):
            i, k = pick[q], int(rng.integers(0, 3))
            j = (k + 1 + int(rng.integers(0, 2))) % 3
            f = int(rng.integers(0, len(AXIS_OFFSETS)))
            sgn = 1.0 if rng.uniform() < 0.5 else -1.0
            o = centers[i].copy()
            o[j] += (1.0 if rng.uniform() < 0.5 else -1.0) * AXIS_OFFSETS[f] * ar[i]
            o[k] -= sgn * (2 * ar[i] + rng.uniform(0, 1) * min(ext, 20 * S))
            out[q, :3] = o
            out[q, 3 + k] = sgn * dlen[q]
            label[q] = f
    elif cls == "zero":
        for q in range(n):
            k = int(rng.integers(0, 3))
            v = ZERO_VALUES[q % 5]
            M = ZERO_ORIGINS[(q // 5) % 5] * (1.0 if rng.uniform() < 0.5 else -1.0)
            f = int(rng.integers(0, 4))                       # the in-plane miss distance: 0, .5, .9 rho or random
            # a sphere that the plane x_k = M cuts, if the scene has one; else a plane through the picked sphere
            cut = np.nonzero(np.abs(centers[:, k] - M) < 0.95 * ar)[0]
            i = int(cut[rng.integers(0, len(cut))]) if len(cut) else int(pick[q])
            ok = M if len(cut) else centers[i, k] + rng.uniform(-0.9, 0.9) * ar[i]
            rho = np.sqrt(max(ar[i] ** 2 - (ok - centers[i, k]) ** 2, 0.0))
            u, w = (k + 1) % 3, (k + 2) % 3
            ang, ang2 = rng.uniform(0, 2 * np.pi, 2)
            tgt = centers[i].copy()
            off = (0.0, 0.5, 0.9, rng.uniform(0, 1.2))[f] * rho
            tgt[u] += off * np.cos(ang2)
            tgt[w] += off * np.sin(ang2)
            d = np.zeros(3)
            d[u], d[w] = np.cos(ang) * dlen[q], np.sin(ang) * dlen[q]
            dist = (2 * ar[i] + rng.uniform(0, 1) * min(ext, 20 * S)) / dlen[q]
            o = tgt - d * dist
            o[k] = ok
            d[k] = v * (1.0 if rng.uniform() < 0.5 else -1.0)
            out[q, :3], out[q, 3:] = o, d
            label[q] = f
    elif cls == "far":
        be = float(grid["far"]) / 64.0 if grid is not None and grid["far"] > 0 else float(np.abs(np.concatenate([lo, hi])).max() + ext)
        u = _unit(rng, n)
        tgt = centers[pick] + 0.5 * ar[pick, None] * _unit(rng, n) * rng.uniform(0, 1, (n, 1))
        fac = np.array(FAR_FACTORS)[np.arange(n) % len(FAR_FACTORS)]
        out[:, :3] = tgt - u * (be * fac)[:, None]
        out[:, 3:] = u * dlen[:, None]
        label = np.arange(n) % len(FAR_FACTORS)
    elif cls == "surface":                                    # continuation rays: leaving (even) and entering (odd)
        nrm = _unit(rng, n)
        d = _unit(rng, n)
        s = np.sign(np.sum(d * nrm, axis=1))
        want = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        d *= (s * want)[:, None]
        out[:, :3] = centers[pick] + ar[pick, None] * nrm
        out[:, 3:] = d * dlen[:, None]
        label = np.arange(n) % 2
    elif cls == "plane":                                      # origins on the cells' binary32 planes lo + k cs
        if grid is not None and int(np.prod(grid["n"])) > 0:
            glo, gcs, gn = (np.asarray(grid[key]) for key in ("lo", "cs", "n"))
        else:
            glo, gcs, gn = lo.astype(np.float32).astype(np.float64), np.maximum((hi - lo) / 4, 1e-30), np.array([4, 4, 4])
        for q in range(n):
            i, a = int(pick[q]), int(rng.integers(0, 3))
            kc = int(np.clip(np.round((centers[i, a] - glo[a]) / gcs[a]), 0, gn[a]))      # the plane nearest the sphere
            zero = rng.uniform() < 0.3 and abs(centers[i, a] - (glo[a] + kc * gcs[a])) < 0.9 * ar[i]
            k = kc if zero or rng.uniform() < 0.5 else int(rng.integers(0, gn[a] + 1))
            plane = float(np.float32(glo[a]) + np.float32(k) * np.float32(gcs[a]))       # binary32 arithmetic
            o = lo + (hi - lo) * rng.uniform(-0.1, 1.1, 3)
            o[a] = plane
            tgt = centers[i] + 0.7 * ar[i] * _unit(rng, 1)[0] * rng.uniform()
            if zero:
                tgt[a] = plane
                rho = np.sqrt(max(ar[i] ** 2 - (plane - centers[i, a]) ** 2, 0.0))
                ang = rng.uniform(0, 2 * np.pi)
                tgt[(a + 1) % 3] = centers[i, (a + 1) % 3] + 0.6 * rho * np.cos(ang)
                tgt[(a + 2) % 3] = centers[i, (a + 2) % 3] + 0.6 * rho * np.sin(ang)
            d = tgt - o
            d *= dlen[q] / max(np.linalg.norm(d), 1e-300)
            if zero:
                d[a] = 0.0
            out[q, :3], out[q, 3:] = o, d
            label[q] = int(zero)
    elif cls == "scaled":                                     # whole directions far from unit length
        o = lo + (hi - lo) * rng.uniform(-0.25, 1.25, (n, 3))
        tgt = centers[pick] + 0.9 * ar[pick, None] * _unit(rng, n) * rng.uniform(0, 1, (n, 1))
        d = tgt - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        sc = np.array(DIR_SCALES)[np.arange(n) % len(DIR_SCALES)]
        out[:, :3], out[:, 3:] = o, d * (S * sc)[:, None]
        label = np.arange(n) % len(DIR_SCALES)
    else:
        raise KeyError(cls)
    return out, label


def all_rays(centers, radii, per_class, seed, grid=None):
    """Every class's rays of a scene: (rays, class index per ray, label per ray)"""
    parts = [rays(c, centers, radii, per_class, seed, grid) for c in RAY_CLASSES]
    return (np.concatenate([p[0] for p in parts]), np.repeat(np.arange(len(RAY_CLASSES)), per_class),
            np.concatenate([p[1] for p in parts]))
