"""Independent reference and inputs for the triangle, box and plane hits (tests/test_tri_walks.py,
test_tri_walks_gpu.py).  Plain NumPy binary64; imports nothing of the project, so a hit query is compared with a
restatement of the reference's World.hit over Sphere, Plane, Box, Triangle and TriangleMesh (js/geometry.js,
js/world.js, js/math.js) and never with another of the project's walks.  TEST INFRASTRUCTURE ONLY.

objects_of(data)       a scene dict's objects as the reference's loader builds them, in World order
world_hit / occluded   the reference's closest hit (t, kind, index) and INTEGRATION.md §8's occlusion rule
tri_hit                Triangle.hit of one triangle alone (the sub-cases that are built to miss their target)
FAMILIES, scene(name)  seeded scenes in the scene-JSON format, each built for something the shipped scenes lack
RAY_CLASSES, all_rays  seeded rays per scene, with a label, the target triangle and a built-to-miss code per ray
"""
import numpy as np

INF = float("inf")
SPHERE, PLANE, BOX, TRI = 0, 1, 2, 3           # rt_closest_hits' kinds; -1: no hit


# ---- the reference's loader (scene-loader.js _createObject, geometry.js constructors) -----------------------------
def _truthy(v):
    if v is None or v is False:
        return False
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return not (v == 0 or v != v)
    if isinstance(v, str):
        return v != ""
    return True


def _num(v):
    return 0.0 if v is None or v is False else 1.0 if v is True else float(v)


def _vec(a):
    return np.array([_num(a[0]), _num(a[1]), _num(a[2])]) if isinstance(a, list) and len(a) >= 3 else np.zeros(3)


def _normalize(v):
    """math.js Vec3.normalize: l = sqrt(x x + y y + z z); l > 0 ? v / l : (0, 0, 0)"""
    l = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return v / l if l > 0 else np.zeros(3)


def _mesh_triangles(vertices, indices):
    """TriangleMesh's constructor: an incomplete triple and one with an index >= vertices.length are skipped; any
    other index that names no vertex (negative, fractional) reads `undefined`, which _ensureVec3 turns into 0."""
    verts = [_vec(v) for v in vertices]
    n = len(verts)
    out = []
    for i in range(0, len(indices), 3):
        if i + 2 >= len(indices):
            continue
        idx = indices[i:i + 3]
        if any(isinstance(x, (int, float)) and not isinstance(x, bool) and x >= n for x in idx):
            continue
        ok = [isinstance(x, (int, float)) and not isinstance(x, bool) and float(x).is_integer() and x >= 0 for x in idx]
        out.append([verts[int(x)] if k else np.zeros(3) for x, k in zip(idx, ok)])
    return np.array(out, dtype=np.float64).reshape(-1, 3, 3)


def objects_of(data):
    """World.objects of a scene dict: a list of (kind, payload, is_mesh): sphere (centre, radius), plane (point,
    normalized normal), box (min, max), triangles (m x 3 x 3 vertices; a standalone triangle has m = 1)."""
    out = []
    for o in data.get("objects") or []:
        if not isinstance(o, dict) or not _truthy(o.get("type")):
            continue
        t = o["type"].lower()
        if t == "sphere":
            r = o.get("radius")
            out.append((SPHERE, (_vec(o.get("center")), _num(r) if _truthy(r) else 1.0), False))
        elif t == "plane":
            out.append((PLANE, (_vec(o.get("point")), _normalize(_vec(o.get("normal")))), False))
        elif t == "box":
            out.append((BOX, (_vec(o.get("min")), _vec(o.get("max"))), False))
        elif t == "triangle":
            out.append((TRI, np.array([[_vec(o.get("v0")), _vec(o.get("v1")), _vec(o.get("v2"))]]), False))
        elif t == "mesh" and _truthy(o.get("vertices")) and _truthy(o.get("indices")):
            out.append((TRI, _mesh_triangles(o["vertices"], o["indices"]), True))
    return out


def triangles_of(objects):
    """Every triangle (T x 3 x 3) in the order of the hit index: World order, mesh triangles in mesh order"""
    parts = [p for k, p, _ in objects if k == TRI]
    return np.concatenate(parts) if parts else np.zeros((0, 3, 3))


# ---- the reference's hit tests ------------------------------------------------------------------------------------
def _js_max(a, b):
    """Math.max: NaN if either is NaN, and +0 above -0"""
    r = np.where(a > b, a, np.where(b > a, b, np.where(np.signbit(a), b, a)))
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def _js_min(a, b):
    """Math.min: NaN if either is NaN, and -0 below +0"""
    r = np.where(a < b, a, np.where(b < a, b, np.where(np.signbit(a), a, b)))
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def _sphere(c, r, R, tmin, tmax):
    ox, oy, oz, dx, dy, dz = R
    a = dx * dx + dy * dy + dz * dz
    ocx, ocy, ocz = ox - c[0], oy - c[1], oz - c[2]
    half_b = ocx * dx + ocy * dy + ocz * dz
    cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r * r
    disc = half_b * half_b - a * cc
    sqrtd = np.sqrt(disc)
    root = (-half_b - sqrtd) / a
    out = (root < tmin) | (tmax < root)
    root = np.where(out, (-half_b + sqrtd) / a, root)
    out = (root < tmin) | (tmax < root)
    return ~(disc < 0) & ~out, root


def _plane(p, n, R, tmin, tmax):
    ox, oy, oz, dx, dy, dz = R
    denom = n[0] * dx + n[1] * dy + n[2] * dz
    t = ((p[0] - ox) * n[0] + (p[1] - oy) * n[1] + (p[2] - oz) * n[2]) / denom
    return ~(np.abs(denom) < 1e-6) & ~((t < tmin) | (t > tmax)), t


def _box(mn, mx, R, tmin, tmax):
    ox, oy, oz, dx, dy, dz = R
    t0, t1 = (mn[0] - ox) / dx, (mx[0] - ox) / dx
    s = t0 > t1
    t0, t1 = np.where(s, t1, t0), np.where(s, t0, t1)
    y0, y1 = (mn[1] - oy) / dy, (mx[1] - oy) / dy
    s = y0 > y1
    y0, y1 = np.where(s, y1, y0), np.where(s, y0, y1)
    ok = ~((t0 > y1) | (y0 > t1))
    t0, t1 = _js_max(t0, y0), _js_min(t1, y1)
    z0, z1 = (mn[2] - oz) / dz, (mx[2] - oz) / dz
    s = z0 > z1
    z0, z1 = np.where(s, z1, z0), np.where(s, z0, z1)
    ok &= ~((t0 > z1) | (z0 > t1))
    t0, t1 = _js_max(t0, z0), _js_min(t1, z1)
    t = np.where(t0 > tmin, t0, t1)
    return ok & ~((t < tmin) | (t > tmax)), t          # a NaN t passes here, and fails World.hit's `<`


def _triangle(v, R, tmin, tmax):
    """Triangle.hit (Möller–Trumbore): products rounded separately, dots summed x, y, z; (hit, t, a)"""
    ox, oy, oz, dx, dy, dz = R
    v0 = v[0]
    e1x, e1y, e1z = v[1] - v0
    e2x, e2y, e2z = v[2] - v0
    hx, hy, hz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
    a = e1x * hx + e1y * hy + e1z * hz
    ok = ~(np.abs(a) < 0.0001)
    f = 1.0 / a
    sx, sy, sz = ox - v0[0], oy - v0[1], oz - v0[2]
    u = f * (sx * hx + sy * hy + sz * hz)
    ok &= ~((u < 0) | (u > 1))
    qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x
    w = f * (dx * qx + dy * qy + dz * qz)
    ok &= ~((w < 0) | (u + w > 1))
    t = f * (e2x * qx + e2y * qy + e2z * qz)
    ok &= ~((t < tmin) | (t > tmax))
    return ok, t, a


def _columns(rays):
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    return tuple(np.ascontiguousarray(rays[:, k]) for k in range(6))


def tri_hit(v, rays, tmin=0.001, tmax=INF):
    """Triangle.hit of the 3 x 3 vertices `v` alone: (hit, t, a = edge1 . (direction x edge2))"""
    with np.errstate(all="ignore"):
        return _triangle(np.asarray(v, dtype=np.float64), _columns(rays), tmin, tmax)


def world_hit(objects, rays, tmin=0.001, tmax=INF):
    """world.js World.hit: (t, kind, index) of n x 6 rays (origin, direction); t = +inf, kind = index = -1 on a miss.
    Objects in World order, each tested against the running closestT and accepted by a strict `<`; a mesh keeps
    a closestT of its own and accepts every hit its triangles report (t <= closestT: the last equal t wins)."""
    R = _columns(rays)
    n = len(R[0])
    closest = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,)).copy()
    best_t = np.full(n, INF)
    best_k = np.full(n, -1, dtype=np.int64)
    best_i = np.full(n, -1, dtype=np.int64)
    count = [0, 0, 0, 0]
    with np.errstate(all="ignore"):
        for kind, p, is_mesh in objects:
            base = count[kind]
            if kind == TRI:
                count[kind] += len(p)
                local = closest.copy()                       # TriangleMesh.hit: closestT = tMax
                hit = np.zeros(n, dtype=bool)
                which = np.full(n, -1, dtype=np.int64)
                for j in range(len(p)):
                    ok, t, _ = _triangle(p[j], R, tmin, local)
                    local = np.where(ok, t, local)
                    which = np.where(ok, base + j, which)
                    hit |= ok
                ok, t, i = hit, local, which
            else:
                count[kind] += 1
                ok, t = (_sphere, _plane, _box)[kind](p[0], p[1], R, tmin, closest)
                i = base
            take = ok & (t < closest)
            closest = np.where(take, t, closest)
            best_t = np.where(take, t, best_t)
            best_k = np.where(take, kind, best_k)
            best_i = np.where(take, i, best_i)
    return best_t, best_k, best_i


def occluded(objects, rays, tmax, tmin=0.001):
    """a shadow ray is occluded iff World.hit(ray, tMin, inf) returns a hit with t < tmax"""
    return world_hit(objects, rays, tmin)[0] < np.asarray(tmax, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- scene families -------------------------------------------------------------------------------------------------
FAMILIES = ("torus", "bowl", "pair", "offset", "tiny", "lattice", "soup", "mixed")
OFFSET = np.array([1000.0, 2000.0, -3000.0])
METAL = {"type": "metal", "color": [0.9, 0.85, 0.7], "roughness": 0.0}
ROUGH = {"type": "metal", "color": [0.8, 0.8, 0.9], "roughness": 0.3}
MATTE = {"type": "lambertian", "color": [0.7, 0.3, 0.3]}
GLASS = {"type": "dielectric", "ior": 1.5}


def _material(rng):
    k = int(rng.integers(0, 10))
    if k < 5:
        return {"type": "lambertian", "color": [float(x) for x in rng.uniform(0.1, 0.9, 3)]}
    if k < 8:
        return {"type": "metal", "color": [float(x) for x in rng.uniform(0.4, 1.0, 3)], "roughness": float(rng.uniform(0, 0.5))}
    return GLASS


def _mesh(verts, idx, material):
    return {"type": "mesh", "vertices": [[float(x) for x in v] for v in verts], "indices": [int(i) for i in idx], "material": material}


def _tri(v0, v1, v2, material):
    return {"type": "triangle", "v0": [float(x) for x in v0], "v1": [float(x) for x in v1], "v2": [float(x) for x in v2],
            "material": material}


def _scene(name, objs, cam_from, cam_at, fov=40.0):
    cam = {"position": [float(x) for x in cam_from], "lookAt": [float(x) for x in cam_at], "up": [0, 1, 0], "fov": fov,
           "aperture": 0.0, "type": "perspective"}
    return {"name": "primitive walks: " + name, "objects": objs, "lights": [], "camera": cam,
            "background": {"type": "gradient", "intensity": 1.0}}


def _grid_indices(nu, nv, wrap_u, wrap_v):
    """two triangles per cell of an nu x nv vertex grid (vertex (i, j) at i * nv + j), wrapping as asked"""
    idx = []
    for i in range(nu if wrap_u else nu - 1):
        for j in range(nv if wrap_v else nv - 1):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            idx += [a, b, d, a, d, c]
    return idx


def torus_mesh(R=1.0, r=0.4, nu=32, nv=20, axis=1, centre=(0.0, 0.0, 0.0)):
    """nu x nv x 2 triangles; the ring lies in the plane normal to `axis`"""
    verts = []
    for i in range(nu):
        for j in range(nv):
            u, v = 2 * np.pi * i / nu, 2 * np.pi * j / nv
            p = [(R + r * np.cos(v)) * np.cos(u), r * np.sin(v), (R + r * np.cos(v)) * np.sin(u)]
            p = p if axis == 1 else [p[1], p[0], p[2]]
            verts.append(np.array(p) + np.array(centre))
    return np.array(verts), _grid_indices(nu, nv, True, True)


def sphere_mesh(radius, nu, nv, centre, lower_only=False):
    """UV sphere; lower_only: the open lower hemisphere (a bowl), its pole a ring of degenerate quads' triangles"""
    verts = []
    rows = nv + 1
    for i in range(nu):
        for j in range(rows):
            th = 2 * np.pi * i / nu
            ph = (np.pi / 2 if lower_only else np.pi) * j / nv            # from the south pole upwards
            verts.append(np.array([radius * np.sin(ph) * np.cos(th), -radius * np.cos(ph), radius * np.sin(ph) * np.sin(th)])
                         + np.array(centre))
    return np.array(verts), _grid_indices(nu, rows, True, False)


def _lattice_objects():
    """Two layers of a checkerboard of unit cells on integer coordinates (z = 0 holds the even cells, z = -1 the
    odd ones), then a coincident copy of the whole mesh with another material, and standalone triangles
    coincident with mesh triangles before and after the first mesh."""
    g = np.arange(-4, 5)
    verts = [[x, y, z] for z in (0, -1) for y in g for x in g]
    at = lambda x, y, layer: layer * 81 + (y + 4) * 9 + (x + 4)
    idx = []
    for y in range(-4, 4):
        for x in range(-4, 4):
            layer = (x + y) % 2
            a, b, c, d = at(x, y, layer), at(x + 1, y, layer), at(x, y + 1, layer), at(x + 1, y + 1, layer)
            idx += [a, b, d, a, d, c]
    verts = np.array(verts, dtype=np.float64)
    tri = lambda k: [verts[i] for i in idx[3 * k:3 * k + 3]]
    before = [_tri(*tri(k), GLASS) for k in (0, 9, 36)]
    after = [_tri(*tri(k), MATTE) for k in (3, 20, 36, 77)]
    return before + [_mesh(verts, idx, METAL)] + after + [_mesh(verts, idx, MATTE)]


def _soup_objects(rng):
    objs = []
    for k in range(300):
        c = rng.uniform(-4, 4, 3)
        size = 10.0 ** rng.uniform(-2, 2)                          # edge lengths over four decades
        a, b = rng.normal(size=3), rng.normal(size=3)
        a, b = a / np.linalg.norm(a) * size, b / np.linalg.norm(b) * size * float(rng.uniform(0.3, 1))
        kind = k % 10
        if kind == 7:
            b = a * 1e-4 + b * 1e-6                                # a needle
        elif kind == 8:
            b = a * float(rng.uniform(0.2, 0.8))                   # collinear: the normal's length is 0
        elif kind == 9:
            a = np.zeros(3)                                        # zero area: v1 == v0
        objs.append(_tri(c, c + a, c + b, _material(rng)))
    v = rng.uniform(-1, 1, (6, 3)) + np.array([0, 5, 0])
    objs.insert(150, _mesh(v, [0, 1, 2, 1, 2, 9, 3, 4, 5, 2, 3, 4, 0, 5], MATTE))       # 9: out of range; 0, 5: incomplete
    return objs


def _mixed_objects(rng):
    tv, ti = torus_mesh(R=1.0, r=0.35, nu=24, nv=12, centre=(0.0, 2.0, 0.0))
    objs = [
        {"type": "plane", "point": [0, 0, 0], "normal": [0, 2, 0], "material": MATTE},               # y = 0
        {"type": "box", "min": [-1, 0, -1], "max": [1, 1, 1], "material": ROUGH},                      # bottom face in the plane
        _tri([-1, 1, -1], [1, 1, -1], [0, 1, 1], GLASS),                                              # in the box's top face, after it
        {"type": "sphere", "center": [2, 0.5, 0], "radius": 1.0, "material": METAL},                  # tangent to the face x = 1
        _mesh(tv, ti, METAL),
        _tri([-3, 0, 2], [-1, 0, 2], [-2, 0, 3], MATTE),                                              # in the plane y = 0, after it
        {"type": "box", "min": [3, 0.5, 3], "max": [4, 0.5, 4], "material": MATTE},                    # min == max on y
        {"type": "box", "min": [-3, 0, 0], "max": [-2, 1, -1], "material": METAL},                     # min > max on z
        {"type": "plane", "point": [0, 0, -6], "normal": [0, 0, 1], "material": ROUGH},
        {"type": "box", "min": [-1, 0, -1], "max": [1, 1, 1], "material": MATTE},                      # coincident with the first box
    ]
    for k in range(12):
        c = rng.uniform(-4, 4, 3) * np.array([1, 0, 1]) + np.array([0, rng.uniform(0.2, 3), 0])
        objs.insert(int(rng.integers(0, len(objs) + 1)),
                    {"type": "sphere", "center": [float(x) for x in c], "radius": float(rng.uniform(0.1, 0.4)), "material": _material(rng)})
    for k in range(12):
        c = rng.uniform(-4, 4, 3) * np.array([1, 0, 1]) + np.array([0, rng.uniform(0.2, 3), 0])
        objs.insert(int(rng.integers(0, len(objs) + 1)), _tri(c, c + rng.uniform(-1, 1, 3), c + rng.uniform(-1, 1, 3), _material(rng)))
    for k in range(4):
        c = rng.uniform(-4, 4, 3) * np.array([1, 0, 1]) + np.array([0, 0.5, 0])
        objs.insert(int(rng.integers(0, len(objs) + 1)),
                    {"type": "box", "min": [float(x) for x in c - rng.uniform(0.1, 0.5, 3)], "max": [float(x) for x in c + rng.uniform(0.1, 0.5, 3)],
                     "material": _material(rng)})
    return objs


def scene(name):
    """The family's scene dict (always the same: each family has its own fixed seed)."""
    rng = np.random.default_rng(2000 + FAMILIES.index(name))
    if name in ("torus", "offset", "tiny"):           # a metal ring linked with a Lambertian one
        parts = [torus_mesh(axis=1), torus_mesh(axis=0, centre=(1.0, 0.0, 0.0))]
        eye, at = np.array([2.5, 2.5, 4.0]), np.array([0.5, 0.0, 0.0])
        if name == "offset":
            parts, eye, at = [(v + OFFSET, i) for v, i in parts], eye + OFFSET, at + OFFSET
        if name == "tiny":                            # hit queries only: tMin = 0.001 swallows a render
            parts, eye, at = [(v * 1e-3, i) for v, i in parts], eye * 1e-3, at * 1e-3
        return _scene(name, [_mesh(*parts[0], METAL), _mesh(*parts[1], MATTE)], eye, at)
    if name == "bowl":
        return _scene(name, [_mesh(*sphere_mesh(1.5, 40, 12, (0.0, 0.0, 0.0), lower_only=True), METAL)], [0.0, 4.0, 2.5], [0, -0.7, 0])
    if name == "pair":
        return _scene(name, [_mesh(*sphere_mesh(1.0, 24, 12, (-1.6, 0.0, 0.0)), METAL),
                             _mesh(*sphere_mesh(0.8, 20, 10, (1.4, 0.3, 0.0)), MATTE)], [0.0, 1.5, 7.0], [0, 0, 0], fov=35.0)
    if name == "lattice":
        return _scene(name, _lattice_objects(), [0.0, 0.0, 12.0], [0, 0, 0])
    if name == "soup":
        return _scene(name, _soup_objects(rng), [1.0, 2.0, 14.0], [0, 0, 0])
    if name == "mixed":
        return _scene(name, _mixed_objects(rng), [3.0, 4.0, 9.0], [0, 1, 0])
    raise KeyError(name)


# ---- ray classes ----------------------------------------------------------------------------------------------------
RAY_CLASSES = ("vertex", "edge", "threshold", "zero", "axis", "surface", "range")
EDGE_POINTS = (0.5, 1e-9, 1 - 1e-9)                                 # along the edge from its first end
THRESHOLD_FACTORS = (1 - 1e-9, 1.0, 1 + 1e-9, 10.0)                 # |a| / 1e-4; the sub-cases below 1 are built to miss
ZERO_VALUES = (0.0, -0.0, 2.0 ** -140, 2.0 ** -120, 2.0 ** -100)    # the replaced direction component
ZERO_ORIGINS = (0.5, 3.9, 4.1, 300.0, 1e4)                          # |origin| on that axis, as tests/sphere_ref.py has them
TMIN_FACTORS = (1 - 1e-9, 1.0, 1 + 1e-9)                            # x tMin along the ray from a triangle's plane
RANGE_D = (2.0 ** -31, 2.0 ** -30, 2.0 ** 30, 2.0 ** 31)            # |d|inf: the pre-filter never rejects outside [2^-30, 2^30]
RANGE_O = (np.nextafter(2.0 ** 30, 0), 2.0 ** 30, np.nextafter(2.0 ** 30, INF))      # |o|inf: never above 2^30


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def aim_triangles(objects):
    """(triangles T x 3 x 3, their hit index or -1): the scene's own triangles, or, in a scene without any, the
    box faces' halves and octahedra inscribed in the spheres, as aim points only"""
    tris = triangles_of(objects)
    if len(tris):
        return tris, np.arange(len(tris))
    out = []
    for kind, p, _ in objects:
        if kind == BOX:
            mn, mx = p
            for a in range(3):                              # each face as two triangles
                b, c = (a + 1) % 3, (a + 2) % 3
                for side in (mn, mx):
                    corner = []
                    for vb, vc in ((mn[b], mn[c]), (mx[b], mn[c]), (mn[b], mx[c]), (mx[b], mx[c])):
                        v = np.zeros(3)
                        v[a], v[b], v[c] = side[a], vb, vc
                        corner.append(v)
                    out += [[corner[0], corner[1], corner[3]], [corner[0], corner[3], corner[2]]]
        elif kind == SPHERE:
            c, r = p
            ax = [c + abs(r) * s * np.eye(3)[k] for k in range(3) for s in (1, -1)]
            out += [[ax[i], ax[2 + j], ax[4 + k]] for i in range(2) for j in range(2) for k in range(2)]
    return np.array(out).reshape(-1, 3, 3), np.full(len(out), -1)


def _good(tris, min_sin=1e-12):
    """indices of the triangles with a normal: |e1 x e2| >= min_sin |e1| |e2| > 0"""
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    nrm = np.linalg.norm(np.cross(e1, e2), axis=1)
    with np.errstate(all="ignore"):
        good = np.nonzero(nrm / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)) >= min_sin)[0]
    return good if len(good) else np.arange(len(tris))


MISS_BUILT, MISS_TARGET = 1, 2
# per ray: 0, or MISS_BUILT for the sub-cases that are built to miss and are left out of a class's hit share (`threshold`
# below 1, unit-scale directions on `tiny`), or MISS_TARGET for rays in their target's own plane (counted in the share);
# either kind must miss the triangle it names


class _Setup:
    """What every class starts from: its own seeded generator, a picked target triangle per ray (vertices T, area
    normal N, unit normal nh), and how the rays approach a target point: from `dist` away with a direction of length
    `dlen`.  tiny: a quarter of the rays keep unit-scale directions (|a| < 1e-4 on every triangle: built to miss);
    the others are long enough for |a|, and start far enough for t >= tMin."""

    def __init__(self, cls, objects, n, seed, tiny):
        self.n, self.tiny = n, tiny
        rng = self.rng = np.random.default_rng(seed + 7919 * RAY_CLASSES.index(cls))
        self.tris, tri_index = aim_triangles(objects)
        # needles are aimed at too, but not where the ray is placed by the triangle's normal (its cross product cancels)
        self.good = _good(self.tris, 1e-3 if cls in ("threshold", "zero") else 1e-12)
        sane = self.tris[self.good]
        box = sane.reshape(-1, 3).max(0) - sane.reshape(-1, 3).min(0)
        edge = float(np.median(np.linalg.norm(sane[:, 1] - sane[:, 0], axis=1)))
        ext = float(min(box.max(), 200 * max(edge, 1e-300)))            # soup: a few huge triangles do not set the scale
        self.boxes = [p for k, p, _ in objects if k == BOX]
        self.pick = self.good[rng.integers(0, len(self.good), n)]
        if not tiny:
            self.dist, self.dlen = ext * rng.uniform(0.5, 3.0, n), 10.0 ** rng.uniform(-1, 1, n)
            self.miss = np.zeros(n, dtype=np.int8)
        else:
            unit = np.arange(n) % 4 == 3
            self.dlen = np.where(unit, 10.0 ** rng.uniform(-1, 0, n), 10.0 ** rng.uniform(5.5, 6.5, n))
            self.dist = np.where(unit, ext * rng.uniform(2.0, 3.0, n), self.dlen * rng.uniform(0.002, 0.02, n))
            self.miss = (unit * MISS_BUILT).astype(np.int8)
        self.label = np.zeros(n, dtype=np.int64)
        self.target = tri_index[self.pick].copy()
        self.T = self.tris[self.pick]
        self.N = np.cross(self.T[:, 1] - self.T[:, 0], self.T[:, 2] - self.T[:, 0])
        self.nh = self.N / np.linalg.norm(self.N, axis=1, keepdims=True)

    def aimed_at(self, p):
        """(origins, directions) of rays through the points p from random sides"""
        o = p - _unit(self.rng, self.n) * self.dist[:, None]
        d = p - o
        return o, d * (self.dlen / np.maximum(np.linalg.norm(d, axis=1), 1e-300))[:, None]

    def inside(self):
        """random points well inside the picked triangles"""
        return np.einsum("nk,nkj->nj", self.rng.dirichlet((2.0, 2.0, 2.0), self.n), self.T)


def _vertex_rays(s):
    return s.aimed_at(s.T[np.arange(s.n), s.rng.integers(0, 3, s.n)])


def _edge_rays(s):
    """label: the point's place in EDGE_POINTS"""
    k = s.rng.integers(0, 3, s.n)
    s.label = np.arange(s.n) % len(EDGE_POINTS)
    a, b = s.T[np.arange(s.n), k], s.T[np.arange(s.n), (k + 1) % 3]
    return s.aimed_at(a + (b - a) * np.array(EDGE_POINTS)[s.label][:, None])


def _threshold_rays(s):
    """a = e1 . (d x e2) = -d . N through the centroid.  Sub-case q % 16: the factor (q % 4), the sign of a, and the
    mode: the direction's length at an elevation of 30 degrees or more (label = factor's place), or the grazing angle
    at the drawn length (label = 4 + place)."""
    n, rng = s.n, s.rng
    q = np.arange(n)
    fac = np.array(THRESHOLD_FACTORS)[q % 4]
    sign = np.where((q // 4) % 2 == 0, 1.0, -1.0)
    graze = (q // 8) % 2 == 1
    s.label = (q % 4) + 4 * graze.astype(np.int64)
    want = 1e-4 * fac
    tang = np.cross(s.nh, _unit(rng, n))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    nn = np.linalg.norm(s.N, axis=1)
    # (no grazing below sin = 1e-3: a's rounding error, 2^-53 / sin relative, must stay far below the factors' 1e-9)
    sin_e = np.where(graze, np.clip(want / (s.dlen * nn), 1e-3, 1.0), np.sin(rng.uniform(np.pi / 6, np.pi / 2, n)))
    dh = tang * np.sqrt(1 - sin_e ** 2)[:, None] - s.nh * (sign * sin_e)[:, None]         # -dh . nh = sign sin_e
    L = want / (nn * sin_e)
    dist = np.maximum(s.dist, L * rng.uniform(0.002, 0.02, n))                            # t >= tMin
    if s.tiny:
        # the well-conditioned sub-case (label 3) starts as near as tMin allows, t = 0.0011 .. 0.0015: binary32 rounds
        # the origin and the direction by 2^-24 of the start distance each, which from farther away is no longer
        # small against a triangle of 10^-4
        dist = np.where(s.label == 3, L * rng.uniform(0.0011, 0.0015, n), dist)
    s.miss = ((fac < 1) * MISS_BUILT).astype(np.int8)          # whatever the family: |d| follows from a
    return s.T.mean(axis=1) - dh * dist[:, None], dh * L[:, None]


def _zero_rays(s):
    """One direction component from ZERO_VALUES, the ray otherwise in the plane x_k = const.  label 0: through the
    picked triangle at its own coordinate, or through one that the plane x_k = +-ZERO_ORIGINS cuts; 1: the origin on a
    box's face plane, aimed across the face (scenes with boxes); 2: in the picked triangle's own plane."""
    rng, tris, good = s.rng, s.tris, s.good
    o, d = np.zeros((s.n, 3)), np.zeros((s.n, 3))
    for q in range(s.n):
        k = int(rng.integers(0, 3))
        u, w = (k + 1) % 3, (k + 2) % 3
        v = ZERO_VALUES[q % 5] * (1.0 if rng.uniform() < 0.5 else -1.0)
        sub = (q // 5) % 3 if s.boxes else 2 * ((q // 5) % 2)
        t = s.T[q]
        ang = rng.uniform(0, 2 * np.pi)
        dq = np.zeros(3)
        dq[u], dq[w] = np.cos(ang), np.sin(ang)
        if sub == 1:
            mn, mx = s.boxes[int(rng.integers(0, len(s.boxes)))]
            tgt = mn + (mx - mn) * rng.uniform(0.1, 0.9, 3)
            tgt[k] = (mn, mx)[int(rng.integers(0, 2))][k]
            s.target[q] = -1
        elif sub == 2:                                        # d = N x e_k
            k = int(np.argmin(np.abs(s.nh[q])))               # never the normal's own axis (N x e_k = 0)
            tgt = t.mean(axis=0)
            dq = np.cross(s.nh[q], np.eye(3)[k])
            dq = dq / max(np.linalg.norm(dq), 1e-300)
            dq[k] = 0.0
            s.miss[q] = s.miss[q] or MISS_TARGET
        else:
            M = ZERO_ORIGINS[(q // 15) % 5] * (1.0 if rng.uniform() < 0.5 else -1.0)
            cut = np.nonzero((tris[good][:, :, k].min(1) < M) & (tris[good][:, :, k].max(1) > M))[0]
            if len(cut) and not s.tiny:
                t = tris[good[cut[int(rng.integers(0, len(cut)))]]]
                s.target[q] = -1
                # a point of the triangle in the plane: on the segment between a vertex below and one above
                lo_v, hi_v = t[np.argmin(t[:, k])], t[np.argmax(t[:, k])]
                tgt = lo_v + (hi_v - lo_v) * ((M - lo_v[k]) / (hi_v[k] - lo_v[k]))
                tgt = tgt + (t.mean(axis=0) - tgt) * 0.01
                tgt[k] = M
            else:
                tgt = t.mean(axis=0)
        oq = tgt - dq * s.dist[q]
        oq[k] = tgt[k]
        dq = dq * s.dlen[q]
        dq[k] = v
        o[q], d[q], s.label[q] = oq, dq, sub
    return o, d


def _axis_rays(s):
    """Axis-aligned.  label 0: through a vertex; 1: an edge's midpoint; 2: the midpoint of v0-v2, which the lattice's
    winding makes a cell's diagonal (elsewhere the centroid); 3: along a box's edge (scenes with boxes)."""
    n, rng, T = s.n, s.rng, s.T
    s.label = np.arange(n) % (4 if s.boxes else 3)
    k = rng.integers(0, 3, n)
    flat = np.abs(s.nh).max(axis=1) > 1 - 1e-12
    p = np.where((s.label == 0)[:, None], T[:, 0], np.where((s.label == 1)[:, None], (T[:, 0] + T[:, 1]) / 2, (T[:, 0] + T[:, 2]) / 2))
    p = np.where(((s.label == 2) & ~flat)[:, None], T.mean(axis=1), p)
    # mostly the axis nearest the normal, so that the ray meets the triangle it names
    k = np.where(rng.uniform(size=n) < 0.7, np.argmax(np.abs(s.nh), axis=1), k)
    for q in np.nonzero(s.label == 3)[0]:
        mn, mx = s.boxes[int(rng.integers(0, len(s.boxes)))]
        c = np.array([(mn, mx)[int(rng.integers(0, 2))][a] for a in range(3)])
        c[k[q]] = mn[k[q]] + (mx[k[q]] - mn[k[q]]) * rng.uniform(0.1, 0.9)
        p[q] = c
        s.target[q] = -1
    sgn = np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0)
    e = np.eye(3)[k]
    return p - e * (sgn * s.dist)[:, None], e * (sgn * s.dlen)[:, None]


def _surface_rays(s):
    """label 0 leaving and 1 entering from a hit point as ray.at(t) computes it; 2..4: the origin tMin x TMIN_FACTORS
    along the ray before the triangle's plane.  tiny: 2..4 only (no second hit can reach tMin there)."""
    n, rng = s.n, s.rng
    s.label = np.arange(n) % 5 if not s.tiny else 2 + np.arange(n) % 3
    p = s.inside()
    o1, d1 = s.aimed_at(p)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for q in range(n):
            if s.label[q] <= 1:
                ok, t1, _ = _triangle(s.T[q], tuple(np.array([x]) for x in (*o1[q], *d1[q])), 0.001, INF)
                t1 = float(t1[0]) if ok[0] else 1.0
                o[q] = o1[q] + d1[q] * t1                                     # ray.at(t): origin + direction * t
                side = -np.sign(np.dot(d1[q], s.nh[q])) or 1.0                # the side the first ray came from
                dq = _unit(rng, 1)[0]
                dq *= np.sign(np.dot(dq, s.nh[q])) * side * (1.0 if s.label[q] == 0 else -1.0)
                d[q] = dq * s.dlen[q]
                s.target[q] = -1
            else:
                d[q] = d1[q]
                o[q] = p[q] - d1[q] * (0.001 * TMIN_FACTORS[s.label[q] - 2])
    return o, d


def _range_rays(s):
    """label 0..3: |d|inf at RANGE_D, from far enough for t >= tMin; 4..6: |o|inf at RANGE_O, the direction at unit
    scale (tiny: 10^6).  tiny: the two small |d| are built to miss (|a| <= 2^-30 |N|)."""
    n = s.n
    s.label = np.arange(n) % 7
    p = s.inside()
    u = _unit(s.rng, n)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for q in range(n):
        if s.label[q] < 4:
            m = RANGE_D[s.label[q]]
            o[q] = p[q] - u[q] * max(s.dist[q], 0.004 * m)
            dq = p[q] - o[q]
            d[q] = dq / np.abs(dq).max() * m
            k = int(np.argmax(np.abs(d[q])))
            d[q, k] = np.sign(d[q, k]) * m
        else:
            m = RANGE_O[s.label[q] - 4]
            oq = p[q] - u[q] * (m / np.abs(u[q]).max())
            k = int(np.argmax(np.abs(oq)))
            oq[k] = np.sign(oq[k]) * m
            o[q] = oq
            d[q] = (p[q] - oq) * ((1e6 if s.tiny else s.dlen[q]) / np.linalg.norm(p[q] - oq))
    s.miss = ((s.label < 2) * MISS_BUILT * int(s.tiny)).astype(np.int8)
    return o, d


_GENERATORS = {"vertex": _vertex_rays, "edge": _edge_rays, "threshold": _threshold_rays, "zero": _zero_rays,
               "axis": _axis_rays, "surface": _surface_rays, "range": _range_rays}


def rays(cls, objects, n, seed, tiny=False):
    """n seeded rays (n x 6) of a class with, per ray, a label (the class's sub-case), the hit index of the triangle
    it was aimed at (-1: none) and 0, MISS_BUILT or MISS_TARGET."""
    s = _Setup(cls, objects, n, seed, tiny)
    o, d = _GENERATORS[cls](s)
    return np.ascontiguousarray(np.concatenate([o, d], axis=1)), s.label, s.target, s.miss


def all_rays(objects, per_class, seed, tiny=False):
    """Every class's rays of a scene: (rays, class index, label, target triangle, built to miss) per ray"""
    parts = [rays(c, objects, per_class, seed, tiny) for c in RAY_CLASSES]
    return (np.concatenate([p[0] for p in parts]), np.repeat(np.arange(len(RAY_CLASSES)), per_class),
            np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]))
