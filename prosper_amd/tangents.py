"""Per-vertex tangents for a primitive that carries none: the rule, stated in NumPy.

prosper generates tangents with mikktspace whenever a primitive has uvs and no TANGENT
(src/scene/DeferredLoadingContext.cpp:843-848).  mikktspace is third-party code that is not in prosper's tree, so the
rule here is the library's own, with mikktspace's convention for w - bitangent = w * cross(n, t), what mapped_normal
computes - and the kernel (csrc/pt_mesh_prepare.hip) reproduces this statement bit for bit.

prosper's flatten-and-reweld is NOT reproduced: vertex count and indices stay as they are.  A vertex that a uv-mirror
seam shares between triangles of both hands therefore gets one tangent, and the hand of the larger sum.

The rule gives the same bits in whatever order the triangles arrive: the per-vertex sum is an integer one.

  per triangle (float32, one rounding per operation, no contraction; division and square root correctly rounded)
      e1 = p1 - p0, e2 = p2 - p0; (s1, t1) = uv1 - uv0, (s2, t2) = uv2 - uv0
      det = s1*t2 - s2*t1
      sdir = (e1*t2 - e2*t1) * sign(det),  tdir = (e2*s1 - e1*s2) * sign(det)
      the triangle contributes nothing unless det, |sdir| and |tdir| are finite and not zero
  per corner (float32)
      weight = the sine of the corner's angle: a, b the two edges that leave the corner, each normalised first (so
      the weight does not depend on the mesh's scale), weight = min(|a^ x b^|, 1); an edge of zero or non-finite
      length contributes nothing
      the corner adds weight * normalize(sdir) and weight * normalize(tdir) to its vertex, each component as fixed
      point: the float32 value times 2^32, exactly, rounded to nearest even, as int64
  per vertex (float64)
      T, B = the int64 sums times 2^-32; n = the vertex normal
      t = normalize(T - n * dot(n, T)); w = -1 if dot(cross(n, t), B) < 0 else +1
      where t has zero or non-finite length: t = normalize(cross(n, axis)), w = +1, axis = the unit axis of n's
      smallest absolute component (the lowest index on a tie); a zero or non-finite n, or a fallback of zero length,
      gives (1, 0, 0, 1)
      the result is rounded to float32

Every dot product is (x*x' + y*y') + z*z', every length sqrt((x*x + y*y) + z*z), every cross product
(a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
"""
import numpy as np

FIXED_ONE = 4294967296.0  # 2^32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _length(a):
    return np.sqrt(_dot(a, a))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def corner_contributions(positions, uvs, indices):
    """-> int64 [m, 3, 6]: what corner c of triangle k adds to its vertex (sdir xyz, tdir xyz), in 2^-32 units."""
    p = np.asarray(positions, np.float32).reshape(-1, 3)
    uv = np.asarray(uvs, np.float32).reshape(-1, 2)
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p0, p1, p2 = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        d1, d2 = uv[tri[:, 1]] - uv[tri[:, 0]], uv[tri[:, 2]] - uv[tri[:, 0]]
        s1, t1, s2, t2 = d1[:, 0:1], d1[:, 1:2], d2[:, 0:1], d2[:, 1:2]
        det = (s1 * t2 - s2 * t1)[:, 0]
        sign = np.where(det < 0, np.float32(-1), np.float32(1))[:, None]
        sdir = (e1 * t2 - e2 * t1) * sign
        tdir = (e2 * s1 - e1 * s2) * sign
        slen, tlen = _length(sdir), _length(tdir)
        valid = np.isfinite(det) & (det != 0) & np.isfinite(slen) & (slen > 0) & np.isfinite(tlen) & (tlen > 0)
        su, tu = sdir / slen[:, None], tdir / tlen[:, None]
        out = np.zeros((len(tri), 3, 6), np.int64)
        for c, (a, b) in enumerate(((e1, e2), (p2 - p1, p0 - p1), (p0 - p2, p1 - p2))):
            la, lb = _length(a), _length(b)
            weight = np.minimum(_length(_cross(a / la[:, None], b / lb[:, None])), np.float32(1))
            ok = valid & np.isfinite(la) & (la > 0) & np.isfinite(lb) & (lb > 0) & np.isfinite(weight)
            value = np.concatenate([su * weight[:, None], tu * weight[:, None]], axis=1)
            assert value.dtype == np.float32
            fixed = np.rint(np.where(ok[:, None], value, np.float32(0)).astype(np.float64) * FIXED_ONE)
            out[:, c] = fixed.astype(np.int64)
    return out


def vertex_sums(vertex_count, indices, contributions):
    """-> int64 [n, 6]: the sums of the corners of every vertex (exact, so in any order)"""
    sums = np.zeros((vertex_count, 6), np.int64)
    np.add.at(sums, np.asarray(indices, np.int64).reshape(-1), contributions.reshape(-1, 6))
    return sums


def finish(sums, normals):
    """int64 sums [n, 6] and the vertex normals -> float32 [n, 4]"""
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        T = sums[:, :3].astype(np.float64) * (1.0 / FIXED_ONE)
        B = sums[:, 3:].astype(np.float64) * (1.0 / FIXED_ONE)
        t = T - n * _dot(n, T)[:, None]
        length = _length(t)
        ok = np.isfinite(length) & (length > 0)
        t = t / length[:, None]
        w = np.where(_dot(_cross(n, t), B) < 0, -1.0, 1.0)
        # the fallback: any unit vector at right angles to the normal
        axis = np.argmin(np.abs(n), axis=1)  # (the first of equal ones)
        x, y, z = n[:, 0], n[:, 1], n[:, 2]
        zero = np.zeros_like(x)
        f = np.where((axis == 0)[:, None], np.stack([zero, z, -y], axis=1),
                     np.where((axis == 1)[:, None], np.stack([-z, zero, x], axis=1), np.stack([y, -x, zero], axis=1)))
        flen = _length(f)
        f = f / flen[:, None]
        fok = np.isfinite(n).all(axis=1) & np.isfinite(flen) & (flen > 0)
        f = np.where(fok[:, None], f, np.array([1.0, 0.0, 0.0]))
        out = np.concatenate([np.where(ok[:, None], t, f), np.where(ok, w, 1.0)[:, None]], axis=1)
    return out.astype(np.float32)


def generate_tangents(positions, normals, uvs, indices):
    """float32 [n, 4] tangents of a primitive with positions [n, 3], normals [n, 3], uvs [n, 2] and triangle indices.
    w follows mikktspace: bitangent = w * cross(normal, tangent.xyz).  Packing is world.pack_snorm3x10_1x2, as for
    supplied tangents."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    return finish(vertex_sums(len(positions), indices, corner_contributions(positions, uvs, indices)), normals)
