"""NumPy restatement of the particle system (res/shader/particles/*, src/render/particles/*): decay, init,
simulate and render in float32 under the arithmetic contract of DESIGN.md section 3, so that the kernels' records and
images can be compared bit for bit.  Slot assignment is not modelled (it depends on the waves' arrival order): the
freelist operations return sets, the callers compare multisets."""
import numpy as np

from prosper_amd import structs as S

F = np.float32
DEAD = F(-9999.0)
GRAVITY, DECAY, EMIT = S.PARTICLE_MASK_GRAVITY, S.PARTICLE_MASK_DECAY, S.PARTICLE_MASK_EMIT

# common/dither.glsl sBayerMatrix, times 64
BAYER64 = np.array([[0, 32, 8, 40, 2, 34, 10, 42], [48, 16, 56, 24, 50, 18, 58, 26], [12, 44, 4, 36, 14, 46, 6, 38],
                    [60, 28, 52, 20, 62, 30, 54, 22], [3, 35, 11, 43, 1, 33, 9, 41], [51, 19, 59, 27, 49, 17, 57, 25],
                    [15, 47, 7, 39, 13, 45, 5, 37], [63, 31, 55, 23, 61, 29, 53, 21]], np.int64)


# ---- float32 arithmetic ----

def fma(a, b, c):
    """fmaf: a * b + c rounded once.  The product of two float32 is exact in float64; the sum is rounded to odd there
    (TwoSum gives its error), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the correct one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    shape = a.shape
    a, b, c = (np.ascontiguousarray(v, F).astype(np.float64).reshape(-1) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        bits = s.view(np.int64)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
        step = np.where((err > 0.0) == (s > 0.0), 1, -1)
        bits = np.where(inexact & ((bits & 1) == 0), bits + step, bits)
        return bits.view(np.float64).astype(F).reshape(shape)


def dot3(a, b):
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def normalize3(v):
    with np.errstate(all="ignore"):
        inv = F(1.0) / np.sqrt(dot3(v, v))
        return (v * inv[..., None]).astype(F)


def saturate(x):
    return np.fmin(np.fmax(x, F(0.0)), F(1.0))  # minNum / maxNum: a NaN operand loses


def pcg3d(v):
    """random.glsl:17-28 on uint32 [n, 3]"""
    v = v.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x, y, z = ((v[:, k] * np.uint64(1664525) + np.uint64(1013904223)) & m for k in range(3))
    x = (x + y * z) & m
    y = (y + z * x) & m
    z = (z + x * y) & m
    x, y, z = x ^ (x >> np.uint64(16)), y ^ (y >> np.uint64(16)), z ^ (z >> np.uint64(16))
    x = (x + y * z) & m
    y = (y + z * x) & m
    z = (z + x * y) & m
    return np.stack([x, y, z], 1).astype(np.uint32)


def rnd3d01(state):
    """-> (rnd3d01() float32 [n, 3], the new state); float(0xFFFFFFFFu) rounds to 2^32"""
    state = pcg3d(state)
    return state.astype(F) / F(4294967296.0), state


# ---- the pool ----

def fresh_pool(n):
    """What Particles::init uploads: (records, count, indices)."""
    rec = np.zeros(n, S.PARTICLE_DTYPE)
    rec["position_lifetime"] = DEAD
    return rec, n, np.arange(n, dtype=np.int32)


def live(records):
    return records["position_lifetime"][:, 3] >= 0.0


def multiset(records):
    """The records' first 52 bytes (the padding is never written), sorted: equal for equal multisets, NaNs included."""
    words = np.ascontiguousarray(records).view(np.uint32).reshape(len(records), 16)[:, :13]
    return words[np.lexsort(words.T[::-1])]


def pop_grants(requesters, free):
    """A launch with k requesters and c free slots grants min(k, c) (f13's dry-freelist rule)."""
    return min(int(requesters), int(free))


# ---- decay.comp ----

def decay(records, decay_all):
    """-> (records after, the slots pushed on the freelist in some order)"""
    out = records.copy()
    lifetime = records["position_lifetime"][:, 3]
    enabled = (records["mask"] & DECAY) != 0
    with np.errstate(invalid="ignore"):
        should = (lifetime != DEAD) & (bool(decay_all) | (enabled & (lifetime <= 0.0)))
    out["position_lifetime"][should] = DEAD
    return out, np.nonzero(should)[0].astype(np.int32)


# ---- init.comp ----

def unpack_snorm(words):
    """geometry.glsl:95-103 on uint32 [n] -> float32 [n, 3]"""
    w = words.astype(np.uint32)
    f = [((w << np.uint32(s)).view(np.int32) >> 22).astype(F) for s in (22, 12, 2)]
    k = F(1.0) / F(511.0)
    return normalize3(np.stack([np.fmax(c * k, F(-1.0)) for c in f], 1))


def init_records(world, draw_instance):
    """The emitter init.comp makes of every vertex of `draw_instance`'s mesh, in vertex order."""
    f = world.freeze()
    di = f["draw_instances"][draw_instance]
    md, info = world.metadatas[di.meshIndex], world.mesh_infos[di.meshIndex]
    n = info.vertexCount
    buf = f["geometry_buffers"][md.bufferIndex]
    half = buf[md.positionsOffset:md.positionsOffset + 2 * n].view(np.float16).reshape(n, 4)
    pm = half[:, :3].astype(F)
    nm = np.zeros((n, 3), F) if md.normalsOffset == S.ABSENT else unpack_snorm(buf[md.normalsOffset:md.normalsOffset + n])
    t = f["transforms"][di.modelInstanceIndex]
    m2w = np.array([[c.x, c.y, c.z, c.w] for c in t.modelToWorld.col], F)
    n2w = np.array([[c.x, c.y, c.z, c.w] for c in t.normalToWorld.col], F)
    # instances.glsl:36-42: vec4(p, 1) * mat3x4 and v * mat3(m)
    pos = np.stack([fma(pm[:, 2], m2w[r, 2], fma(pm[:, 1], m2w[r, 1], fma(pm[:, 0], m2w[r, 0], m2w[r, 3]))) for r in range(3)], 1)
    nrm = normalize3(np.stack([fma(nm[:, 2], n2w[r, 2], fma(nm[:, 1], n2w[r, 1], nm[:, 0] * n2w[r, 0])) for r in range(3)], 1))
    rec = np.zeros(n, S.PARTICLE_DTYPE)
    rec["position_lifetime"][:, :3] = pos
    rec["normal_spawnRateS"][:, :3] = nrm
    rec["normal_spawnRateS"][:, 3] = F(0.1)
    rec["mask"] = EMIT
    return rec


# ---- simulate.comp ----

def simulate(records, dt, frame_index):
    """-> (the pool's records after the step, children, parents): `children` are the records the emitters in `parents`
    (slot indices, ascending) spawn, one each, before any of them is refused."""
    dt = F(dt)
    n = len(records)
    out = records.copy()
    slot = np.arange(n, dtype=np.uint32)
    pl, ns, vs = (records[k].astype(F) for k in ("position_lifetime", "normal_spawnRateS", "velocity_spawnTimerS"))
    mask = records["mask"]
    with np.errstate(all="ignore"):
        run = ~(pl[:, 3] < 0.0)
        position = (pl[:, :3] + vs[:, :3] * dt).astype(F)
        velocity = vs[:, :3].copy()
        lifetime = pl[:, 3].copy()
        timer = vs[:, 3].copy()
        g = (mask & GRAVITY) != 0
        velocity[g, 1] = velocity[g, 1] - (F(9.81) * F(0.01)) * dt
        d = (mask & DECAY) != 0
        lifetime[d] = lifetime[d] - dt
        e = ((mask & EMIT) != 0) & run
        r, _ = rnd3d01(np.stack([slot, slot % np.uint32(256), np.full(n, frame_index, np.uint32)], 1))
        normal = ns[:, :3]
        push = ((((normal + r * F(2.0)) - F(1.0)) * F(0.5)) * dt).astype(F)
        ve = (velocity + push).astype(F)
        scalar = np.sqrt(dot3(ve, ve))
        ve = (ve * (F(1.0) / scalar)[:, None]).astype(F)
        scalar = np.fmin(scalar, F(0.05))
        ve = (ve * scalar[:, None]).astype(F)
        ne = normalize3(ve)
        te = (timer + dt).astype(F)
        spawn = e & (te >= ns[:, 3])
        te[spawn] = F(0.0)
        velocity[e] = ve[e]
        timer[e] = te[e]
        out["normal_spawnRateS"][e, :3] = ne[e]
        out["position_lifetime"][run, :3] = position[run]
        out["position_lifetime"][run, 3] = lifetime[run]
        out["velocity_spawnTimerS"][run, :3] = velocity[run]
        out["velocity_spawnTimerS"][run, 3] = timer[run]
        parents = np.nonzero(spawn)[0]
        children = np.zeros(len(parents), S.PARTICLE_DTYPE)
        children["position_lifetime"][:, :3] = position[parents]
        children["position_lifetime"][:, 3] = F(4.0)
        children["normal_spawnRateS"][:, :3] = ne[parents]
        children["velocity_spawnTimerS"][:, :3] = ((ne[parents] * scalar[parents, None]).astype(F) * F(2.0)).astype(F)
        children["mask"] = GRAVITY | DECAY
    return out, children, parents


# ---- render.vert / rasterisation / render.frag ----

def mat4(m):
    """S.Mat4 -> float32 [row, column]"""
    return np.array([[getattr(m.col[c], "xyzw"[r]) for c in range(4)] for r in range(4)], F)


def world_to_clip(camera):
    """cameraToClip * worldToCamera in float64, summed in k order, rounded once: what the traced G-buffer's depth uses"""
    a, b = mat4(camera.cameraToClip).astype(np.float64), mat4(camera.worldToCamera).astype(np.float64)
    out = np.zeros((4, 4), np.float64)
    for r in range(4):
        for c in range(4):
            v = 0.0
            for k in range(4):
                v += a[r, k] * b[k, c]
            out[r, c] = v
    return out.astype(F)


def camera_axes(camera):
    """normalize(cameraWorldUp()), normalize(cameraWorldRight()) of scene/camera.glsl:32-44"""
    w2c = mat4(camera.worldToCamera)
    return normalize3(w2c[1, :3].copy()), normalize3((-w2c[0, :3]).astype(F))


def clip_row(m, row, p):
    return fma(m[row, 2], p[..., 2], fma(m[row, 1], p[..., 1], fma(m[row, 0], p[..., 0], m[row, 3])))


def quad_corners(position, camera, width, height):
    """-> (depth, X int64 [4], Y int64 [4]) of the quad around `position` in 1/256 pixels, or None when the quad is
    dropped whole (w <= 0, depth outside [0, 1], a coordinate beyond 2^23)."""
    m = world_to_clip(camera)
    up, right = camera_axes(camera)
    centre = np.asarray(position, F)
    with np.errstate(all="ignore"):
        w = clip_row(m, 3, centre)
        if not w > 0.0:
            return None
        depth = F(clip_row(m, 2, centre) / w)
        if not (depth >= 0.0 and depth <= 1.0):
            return None
        X, Y = [], []
        for k in range(4):
            xo = F(0.001) if k & 1 else F(-0.001)
            yo = F(-0.001) if k & 2 else F(0.001)
            p = (centre + up * yo).astype(F)
            p = (p + right * xo).astype(F)
            cw = clip_row(m, 3, p)
            fx = F((F(clip_row(m, 0, p) / cw) * F(0.5) + F(0.5)) * F(width))
            fy = F((F(clip_row(m, 1, p) / cw) * F(0.5) + F(0.5)) * F(height))
            sx, sy = np.rint(F(fx * F(256.0))), np.rint(F(fy * F(256.0)))
            if not (abs(sx) <= 8388608.0 and abs(sy) <= 8388608.0):
                return None
            X.append(int(sx))
            Y.append(int(sy))
    return depth, X, Y


def triangle_area2(X, Y, tri):
    """Twice the signed area in framebuffer coordinates (y down).  Vulkan's a is -1/2 of it: negative here = front."""
    (ax, ay), (bx, by), (cx, cy) = ((X[i], Y[i]) for i in tri)
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


STRIP = ((0, 1, 2), (2, 1, 3))


def quad_coverage(X, Y, width, height):
    """Pixels (py, px arrays) whose centres the strip's two front-facing triangles cover under the top-left rule."""
    px0, px1 = max(0, (min(X) + 127) >> 8), min(width - 1, (max(X) - 128) >> 8)
    py0, py1 = max(0, (min(Y) + 127) >> 8), min(height - 1, (max(Y) - 128) >> 8)
    if px0 > px1 or py0 > py1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    py, px = np.mgrid[py0:py1 + 1, px0:px1 + 1].astype(np.int64)
    sx, sy = px * 256 + 128, py * 256 + 128
    covered = np.zeros(px.shape, bool)
    for tri in STRIP:
        if triangle_area2(X, Y, tri) >= 0:
            continue  # back-facing or empty
        inside = np.ones(px.shape, bool)
        for e in range(3):
            a, b = tri[e], tri[(e + 1) % 3]
            ex, ey = X[b] - X[a], Y[b] - Y[a]
            f = ey * (sx - X[a]) - ex * (sy - Y[a])
            top_left = ey > 0 or (ey == 0 and ex < 0)
            inside &= (f > 0) | ((f == 0) & top_left)
        assert not (covered & inside).any()  # the fill rule gives a pixel on the diagonal to one triangle
        covered |= inside
    return py[covered], px[covered]


def dither_passes(alpha, py, px, frame_index):
    """render.frag: step(threshold, alpha) with the matrix cycled by the frame index"""
    threshold = BAYER64[(py + frame_index // 8) % 8, (px + frame_index % 8) % 8].astype(F) * F(1.0 / 64.0)
    return ~(F(alpha) < threshold)


def render(records, camera, width, height, frame_index, hdr, depth):
    """-> (hdr, depth, fragments): the images after the pass and, per slot, how many pixels it owns in the end."""
    out_hdr, out_depth = hdr.copy(), depth.copy()
    best = np.zeros((height, width), F)       # the winning depth per pixel ...
    owner = np.full((height, width), -1, np.int64)  # ... and its slot
    for slot in np.nonzero(live(records))[0]:
        rec = records[slot]
        q = quad_corners(rec["position_lifetime"][:3], camera, width, height)
        if q is None:
            continue
        d, X, Y = q
        py, px = quad_coverage(X, Y, width, height)
        emitter = bool(rec["mask"] & EMIT)
        alpha = F(1.0) if emitter else saturate(F(rec["position_lifetime"][3] * F(4.0)))
        keep = dither_passes(alpha, py, px, frame_index)
        py, px = py[keep], px[keep]
        with np.errstate(invalid="ignore"):
            passes = d > depth[py, px]  # strict, against the stored depth
            wins = passes & ((owner[py, px] < 0) | (d > best[py, px]))  # equal depths: the lower slot came first
        py, px = py[wins], px[wins]
        best[py, px] = d
        owner[py, px] = slot
    fragments = np.zeros(len(records), np.int64)
    hit = owner >= 0
    if hit.any():
        emit = (records["mask"][owner[hit]] & EMIT) != 0
        out_hdr[hit] = np.where(emit[:, None], np.array([1, 1, 0, 1], F), np.array([1, 0, 1, 1], F))
        out_depth[hit] = best[hit]
        np.add.at(fragments, owner[hit], 1)
    return out_hdr, out_depth, fragments
