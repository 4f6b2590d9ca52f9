"""NumPy restatement of the keyframe animation (prosper_amd/csrc/pt_animation.hip), one operation per
rounding: `TimeAccessor::interpolation` + `Animation<T>::update` (kernel A) and the scene-graph walk with glm's
translate / mat4_cast / scale / inverse (kernel B), over the tables of `prosper_amd.animation`.  `f` is the float type:
np.float32 restates the kernels bit for bit (but for the two transcendentals of slerp, which belong to each libm),
np.float64 is the yardstick for slerp's error.  Matrices are m[column][row], quaternions (x, y, z, w)."""
import numpy as np

from prosper_amd import structs as S

NONE = S.ANIMATION_NONE
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
_FLAG = {S.ANIMATION_PATH_TRANSLATION: S.NODE_HAS_TRANSLATION, S.ANIMATION_PATH_ROTATION: S.NODE_HAS_ROTATION,
         S.ANIMATION_PATH_SCALE: S.NODE_HAS_SCALE}
_SLOT = {S.ANIMATION_PATH_TRANSLATION: slice(0, 3), S.ANIMATION_PATH_ROTATION: slice(3, 7), S.ANIMATION_PATH_SCALE: slice(7, 10)}


# ---------------------------------------------------------------------------------------------------------------------
# kernel A
# ---------------------------------------------------------------------------------------------------------------------

def first_frame_linear(times, time_s):
    """The reference's scan (Accessors.cpp:45-57) for a time past the early-outs."""
    last = len(times) - 1
    first = 0
    while first < last:
        if times[first] > time_s:
            break
        first += 1
    return first - 1


def first_frame_binary(times, time_s):
    """The kernel's search: the first frame in [0, last) whose time exceeds time_s (or last), minus one."""
    lo, hi = 0, len(times) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if times[mid] > time_s:
            hi = mid
        else:
            lo = mid + 1
    return lo - 1


def key_frame(times, start, end, time_s, f=np.float32, search=first_frame_binary):
    """(t, stepDuration, firstFrame) of TimeAccessor::interpolation."""
    times = np.asarray(times, f)
    time_s, zero = f(time_s), f(0.0)
    if time_s <= f(start) or time_s < times[0]:
        return zero, zero, 0
    last = len(times) - 1
    if time_s >= f(end) or last == 0:
        return zero, zero, last
    first = search(times, time_s)
    duration = times[first + 1] - times[first]
    step = time_s - times[first]  # the time since the key, not the key interval
    with np.errstate(divide="ignore", invalid="ignore"):
        return step / duration, step, first


def quat_dot(a, b):
    return (a[3] * b[3] + a[0] * b[0]) + (a[1] * b[1] + a[2] * b[2])


def slerp_branch(x, y):
    """'mix' or 'slerp': which branch glm::slerp takes for the float32 keys x, y."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    cos_theta = quat_dot(x, y)
    if cos_theta < 0:
        cos_theta = -cos_theta
    return "mix" if cos_theta > np.float32(1.0) - FLT_EPSILON else "slerp"


def slerp(x, y, a, f=np.float32):
    """glm::slerp.  The branch is the float32 one in either mode: the yardstick follows the kernel's path."""
    branch = slerp_branch(x, y)
    x, y, a = np.asarray(x, f), np.asarray(y, f), f(a)
    z = y
    cos_theta = quat_dot(x, y)
    if quat_dot(np.asarray(x, np.float32), np.asarray(y, np.float32)) < 0:
        z = -y
        cos_theta = -cos_theta
    if branch == "mix":
        return x * (f(1.0) - a) + z * a
    angle = np.arccos(cos_theta)
    return (np.sin((f(1.0) - a) * angle) * x + np.sin(a * angle) * z) / np.sin(angle)


def channel_values(tables, ch):
    width = 4 if ch.path == S.ANIMATION_PATH_ROTATION else 3
    per_key = 3 if ch.interpolation == S.ANIMATION_CUBICSPLINE else 1
    n = ch.keyCount * per_key * width
    return tables.values[ch.valueOffset:ch.valueOffset + n].reshape(ch.keyCount * per_key, width)


def channel_times(tables, ch):
    return tables.times[ch.timeOffset:ch.timeOffset + ch.keyCount]


def sample_channel(tables, ch, time_s, f=np.float32):
    """Animation<T>::update: the value the channel writes at time_s."""
    v = channel_values(tables, ch).astype(f)
    quat = ch.path == S.ANIMATION_PATH_ROTATION
    t, td, first = key_frame(channel_times(tables, ch), ch.startTimeS, ch.endTimeS, time_s, f)
    cubic = ch.interpolation == S.ANIMATION_CUBICSPLINE
    one, two, three = f(1.0), f(2.0), f(3.0)
    if t == 0 or ch.interpolation == S.ANIMATION_STEP:
        return v[first * 3 + 1] if (t == 0 and cubic) else v[first]
    if ch.interpolation == S.ANIMATION_LINEAR:
        if quat:
            return slerp(v[first], v[first + 1], t, f)
        return (one - t) * v[first] + t * v[first + 1]
    i = first * 3
    vk, bk, vk1, ak1 = v[i + 1], v[i + 2], v[i + 4], v[i + 3]
    t3, t2, t2x2, t3x2, t2x3 = t * t * t, t * t, two * t * t, two * t * t * t, three * t * t
    value = (t3x2 - t2x3 + one) * vk + (td * (t3 - t2x2 + t)) * bk + (-t3x2 + t2x3) * vk1 + (td * (t3 - t2)) * ak1
    if quat:
        length = np.sqrt(quat_dot(value, value))
        if length <= 0:
            return np.array([0, 0, 0, 1], f)
        value = value * (one / length)
    return value


def resolve_targets(tables):
    """{(node, path): channel}: where several channels target one (node, path) the last one wins."""
    winner = {}
    for ch in tables.channels:
        winner[(ch.node, ch.path)] = ch
    return winner


def static_pose(tables):
    """(flags [n], trs [n, 10] float32): a targeted component exists, and starts at the identity if it had been dropped."""
    n = len(tables.nodes)
    flags = np.array([nd.flags for nd in tables.nodes], np.uint32)
    trs = np.zeros((n, 10), np.float32)
    for i, nd in enumerate(tables.nodes):
        trs[i] = list(nd.translation) + list(nd.rotation) + list(nd.scale)
    identity = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1], np.float32)
    for (node, path) in resolve_targets(tables):
        if not flags[node] & _FLAG[path]:
            flags[node] |= _FLAG[path]
            trs[node, _SLOT[path]] = identity[_SLOT[path]]
    return flags, trs


def evaluate_trs(tables, time_s, f=np.float32):
    """Kernel A: the per-node translation / rotation / scale at time_s, [n, 10]."""
    _, trs = static_pose(tables)
    trs = trs.astype(f)
    for (node, path), ch in resolve_targets(tables).items():
        trs[node, _SLOT[path]] = sample_channel(tables, ch, time_s, f)
    return trs


def dynamic_nodes(tables):
    """Per node: a channel targets it or one of its ancestors (WorldData.cpp:1279-1320)."""
    dyn = [False] * len(tables.nodes)
    for (node, _) in resolve_targets(tables):
        dyn[node] = True
    for i, nd in enumerate(tables.nodes):
        if nd.parent != NONE:
            dyn[i] = dyn[i] or dyn[nd.parent]
    return dyn


# ---------------------------------------------------------------------------------------------------------------------
# kernel B
# ---------------------------------------------------------------------------------------------------------------------

def translate(m, v):
    out = m.copy()
    out[3] = m[0] * v[0] + m[1] * v[1] + m[2] * v[2] + m[3]
    return out


def mat4_cast(q, f):
    x, y, z, w = q
    one, two = f(1.0), f(2.0)
    xx, yy, zz, xz, xy, yz, wx, wy, wz = x * x, y * y, z * z, x * z, x * y, y * z, w * x, w * y, w * z
    b = np.zeros((4, 4), f)
    b[0, :3] = [one - two * (yy + zz), two * (xy + wz), two * (xz - wy)]
    b[1, :3] = [two * (xy - wz), one - two * (xx + zz), two * (yz + wx)]
    b[2, :3] = [two * (xz + wy), two * (yz - wx), one - two * (xx + yy)]
    b[3, 3] = one
    return b


def mat_mul(a, b):
    out = np.empty_like(a)
    for j in range(4):
        out[j] = a[0] * b[j, 0] + a[1] * b[j, 1] + a[2] * b[j, 2] + a[3] * b[j, 3]
    return out


def scale(m, v):
    out = m.copy()
    for j in range(3):
        out[j] = m[j] * v[j]
    return out


def inverse(m, f):
    """glm::inverse of a mat4: cofactors, one division."""
    c = lambda a, b, cc, d: m[a[0], a[1]] * m[b[0], b[1]] - m[cc[0], cc[1]] * m[d[0], d[1]]  # noqa: E731
    coef00 = c((2, 2), (3, 3), (3, 2), (2, 3))
    coef02 = c((1, 2), (3, 3), (3, 2), (1, 3))
    coef03 = c((1, 2), (2, 3), (2, 2), (1, 3))
    coef04 = c((2, 1), (3, 3), (3, 1), (2, 3))
    coef06 = c((1, 1), (3, 3), (3, 1), (1, 3))
    coef07 = c((1, 1), (2, 3), (2, 1), (1, 3))
    coef08 = c((2, 1), (3, 2), (3, 1), (2, 2))
    coef10 = c((1, 1), (3, 2), (3, 1), (1, 2))
    coef11 = c((1, 1), (2, 2), (2, 1), (1, 2))
    coef12 = c((2, 0), (3, 3), (3, 0), (2, 3))
    coef14 = c((1, 0), (3, 3), (3, 0), (1, 3))
    coef15 = c((1, 0), (2, 3), (2, 0), (1, 3))
    coef16 = c((2, 0), (3, 2), (3, 0), (2, 2))
    coef18 = c((1, 0), (3, 2), (3, 0), (1, 2))
    coef19 = c((1, 0), (2, 2), (2, 0), (1, 2))
    coef20 = c((2, 0), (3, 1), (3, 0), (2, 1))
    coef22 = c((1, 0), (3, 1), (3, 0), (1, 1))
    coef23 = c((1, 0), (2, 1), (2, 0), (1, 1))
    v4 = lambda *a: np.array(a, f)  # noqa: E731
    fac0, fac1, fac2 = v4(coef00, coef00, coef02, coef03), v4(coef04, coef04, coef06, coef07), v4(coef08, coef08, coef10, coef11)
    fac3, fac4, fac5 = v4(coef12, coef12, coef14, coef15), v4(coef16, coef16, coef18, coef19), v4(coef20, coef20, coef22, coef23)
    vec0, vec1 = v4(m[1, 0], m[0, 0], m[0, 0], m[0, 0]), v4(m[1, 1], m[0, 1], m[0, 1], m[0, 1])
    vec2, vec3 = v4(m[1, 2], m[0, 2], m[0, 2], m[0, 2]), v4(m[1, 3], m[0, 3], m[0, 3], m[0, 3])
    sign_a, sign_b = v4(1, -1, 1, -1), v4(-1, 1, -1, 1)
    inv = np.empty((4, 4), f)
    inv[0] = (vec1 * fac0 - vec2 * fac1 + vec3 * fac2) * sign_a
    inv[1] = (vec0 * fac0 - vec2 * fac3 + vec3 * fac4) * sign_b
    inv[2] = (vec0 * fac1 - vec1 * fac3 + vec3 * fac5) * sign_a
    inv[3] = (vec0 * fac2 - vec1 * fac4 + vec2 * fac5) * sign_b
    dot0 = m[0] * inv[:, 0]
    dot1 = (dot0[0] + dot0[1]) + (dot0[2] + dot0[3])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return inv * (f(1.0) / dot1)


def mat_mul_vec4(m, v):
    return (m[0] * v[0] + m[1] * v[1]) + (m[2] * v[2] + m[3] * v[3])


def mat3_mul_vec3(m, v):
    return (m[0] * v[0] + m[1] * v[1] + m[2] * v[2])[:3]


def hierarchy(tables, trs, f=np.float32):
    """World matrices [n, 4, 4] (m[column][row]) from the per-node TRS: for each ancestor from the root down and then the
    node itself translate, *= mat4_cast, scale - for the components the node has."""
    flags, _ = static_pose(tables)
    trs = np.asarray(trs, f)
    world = np.zeros((len(tables.nodes), 4, 4), f)
    for i, nd in enumerate(tables.nodes):
        m = np.eye(4, dtype=f) if nd.parent == NONE else world[nd.parent].copy()
        # (the chain from the root re-done per node in the kernel gives the parent's matrix at every step: same operations)
        if flags[i] & S.NODE_HAS_TRANSLATION:
            m = translate(m, trs[i, 0:3])
        if flags[i] & S.NODE_HAS_ROTATION:
            m = mat_mul(m, mat4_cast(trs[i, 3:7], f))
        if flags[i] & S.NODE_HAS_SCALE:
            m = scale(m, trs[i, 7:10])
        world[i] = m
    return world


def outputs(tables, world, transforms, directional, points, spots):
    """What kernel B writes from the world matrices, over copies of the inputs: the ModelInstanceTransforms table as
    [instances, 2, 3, 4] float32 (modelToWorld, normalToWorld; column, component), the directional light's direction [4],
    the point lights' positions [count, 4], the spot lights as [count, 2, 4] (positionAndAngleOffset, direction), and the
    camera record [9] (or None).  World.cpp:405-457."""
    f = world.dtype.type
    table = np.array(transforms, np.float32, copy=True)
    directional, points, spots = (np.array(a, np.float32, copy=True) for a in (directional, points, spots))
    camera = None
    zero, one = f(0.0), f(1.0)
    for i, nd in enumerate(tables.nodes):
        m = world[i]
        if nd.modelInstance != NONE:
            table[nd.modelInstance, 0] = m.T[:3]           # mat3x4(transpose(M))
            table[nd.modelInstance, 1] = inverse(m, f)[:3]  # mat3x4(inverse(M))
        position = mat_mul_vec4(m, [zero, zero, zero, one])
        direction = mat3_mul_vec3(m, [zero, zero, -one])
        if nd.flags & S.NODE_DIRECTIONAL_LIGHT:
            directional[:3], directional[3] = direction, 0.0
        if nd.pointLight != NONE:
            points[nd.pointLight] = position
        if nd.spotLight != NONE:
            spots[nd.spotLight, 0, :3] = position[:3]
            spots[nd.spotLight, 1, :3], spots[nd.spotLight, 1, 3] = direction, 0.0
        if nd.flags & S.NODE_CAMERA:
            camera = np.concatenate([position[:3], mat_mul_vec4(m, [zero, zero, -one, one])[:3],
                                     mat3_mul_vec3(m, [zero, one, zero])]).astype(np.float32)
    return table, directional, points, spots, camera


# ---------------------------------------------------------------------------------------------------------------------
# the tests' case lists
# ---------------------------------------------------------------------------------------------------------------------

def sample_times(tables, seed=15, random_count=64):
    """Before every start, exactly on keys, strictly between keys, at endTimeS, beyond it, and seeded random times."""
    end = tables.end_time
    times = [-1.0, 0.0, end, end + 1.0]
    for ch in tables.channels:
        t = channel_times(tables, ch)
        times += [float(x) for x in t]
        times += [float(np.float32(0.5) * (a + b)) for a, b in zip(t[:-1], t[1:]) if b > a]
        times += [float(ch.startTimeS), float(ch.endTimeS)]
    rng = np.random.default_rng(seed)
    times += [float(x) for x in rng.uniform(0.0, end, random_count).astype(np.float32)]
    return sorted(set(float(np.float32(t)) for t in times))


def slerp_samples(tables, times):
    """Every (x, y, a) a winning LINEAR rotation channel hands slerp over `times`, with its branch."""
    out = []
    for (node, path), ch in resolve_targets(tables).items():
        if path != S.ANIMATION_PATH_ROTATION or ch.interpolation != S.ANIMATION_LINEAR:
            continue
        v = channel_values(tables, ch)
        for time_s in times:
            t, _, first = key_frame(channel_times(tables, ch), ch.startTimeS, ch.endTimeS, time_s)
            if t != 0:
                out.append((v[first], v[first + 1], t, slerp_branch(v[first], v[first + 1])))
    return out


def slerp_error(tables, times):
    """E_ref: the largest component difference between the float32 and the float64 restatement over slerp_samples."""
    worst = 0.0
    for x, y, a, _ in slerp_samples(tables, times):
        worst = max(worst, float(np.max(np.abs(slerp(x, y, a, np.float32).astype(np.float64) - slerp(x, y, a, np.float64)))))
    return worst
