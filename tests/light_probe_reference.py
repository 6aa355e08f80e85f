"""The light probes' projection as the header defines it (include/srt_pathtrace.h, the light-probe block, rules 3-5), in numpy
float32: the nine basis values, the term, the sum over blocks of 64 directions with a pairwise tree of six levels inside a block
and an ascending fold across blocks; the irradiance formula of srt_light_probe_irradiance; the spherical Fibonacci set of
srt_light_probe_sphere.  Not a test: tests/test_light_probe_reference.py and tests/test_gpu_light_probes.py import it."""
import numpy as np

F = np.float32
COEFFS = 9


def basis(d):
    """(K, 9) float32 basis values on the directions d (K, >= 3), in the header's expressions."""
    d = np.asarray(d, dtype=F)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    b = np.empty((d.shape[0], COEFFS), dtype=F)
    b[:, 0] = F(0.282095)
    b[:, 1] = F(0.488603) * y
    b[:, 2] = F(0.488603) * z
    b[:, 3] = F(0.488603) * x
    b[:, 4] = F(1.092548) * (x * y)
    b[:, 5] = F(1.092548) * (y * z)
    b[:, 6] = F(0.315392) * ((F(3.0) * (z * z)) - F(1.0))
    b[:, 7] = F(1.092548) * (x * z)
    b[:, 8] = F(0.546274) * ((x * x) - (y * y))
    return b


def terms(directions):
    """t[k, c] = w_k * b_c(d_k), float32 (K, 9); directions (K, 4) as traced, the weight in w."""
    d = np.asarray(directions, dtype=F)
    return (d[:, 3:4] * basis(d)).astype(F)


def lane_values(radiance, directions):
    """v[p, k, c, :] = (L.r t, L.g t, L.b t, t): radiance (P, K, 4), directions (K, 4) -> (P, K, 9, 4) float32."""
    L = np.asarray(radiance, dtype=F)
    t = terms(directions)
    v = np.empty(L.shape[:2] + (COEFFS, 4), dtype=F)
    v[..., :3] = L[:, :, None, :3] * t[None, :, :, None]
    v[..., 3] = t[None, :, :]
    return v


def tree_sum(v):
    """The header's sum order over axis 1 of v (P, K, ...): blocks of 64, positions past K are +0, a pairwise tree of six levels
    inside a block (v'[m] = v[2m] + v[2m+1]), then S = B_0, S = S + B_j ascending."""
    v = np.asarray(v, dtype=F)
    P, K = v.shape[:2]
    J = (K + 63) // 64
    pad = np.zeros((P, J * 64) + v.shape[2:], dtype=F)
    pad[:, :K] = v
    b = pad.reshape((P, J, 64) + v.shape[2:])
    for _ in range(6):
        b = (b[:, :, 0::2] + b[:, :, 1::2]).astype(F)
    b = b[:, :, 0]
    s = b[:, 0].copy()
    for j in range(1, J):
        s = (s + b[:, j]).astype(F)
    return s


def left_to_right_sum(v):
    """The sum a plain loop over k would give: for the order-sensitivity test only."""
    v = np.asarray(v, dtype=F)
    s = v[:, 0].copy()
    for k in range(1, v.shape[1]):
        s = (s + v[:, k]).astype(F)
    return s


def project(radiance, directions):
    """(P, 9, 4) float32 coefficients of radiance (P, K, 4) over the directions (K, 4) as traced."""
    return tree_sum(lane_values(radiance, directions))


A = np.array([3.14159274] + [2.09439516] * 3 + [0.785398185] * 5, dtype=F)


def irradiance(coefficients, normal):
    """rgb (3,) float32: term_c = (A_c * coefficient_c[l]) * b_c(n), E = term_0, E = E + term_c ascending."""
    c = np.asarray(coefficients, dtype=F).reshape(COEFFS, 4)
    b = basis(np.asarray(normal, dtype=F).reshape(1, -1))[0]
    out = np.empty(3, dtype=F)
    for l in range(3):
        e = F((A[0] * c[0, l]) * b[0])
        for k in range(1, COEFFS):
            e = F(e + F(F(A[k] * c[k, l]) * b[k]))
        out[l] = e
    return out


def sphere(count):
    """The spherical Fibonacci set in float64, rounded once: (count, 4) float32."""
    i = np.arange(count, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / count
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    a = i * (np.pi * (3.0 - np.sqrt(5.0)))
    out = np.empty((count, 4), dtype=F)
    out[:, 0], out[:, 1], out[:, 2] = r * np.cos(a), r * np.sin(a), z
    out[:, 3] = F(4.0 * np.pi / count)
    return out


def normalized(directions):
    """float3::Normalized on the xyz of (K, 4) directions, as the kernel computes it for finite non-tiny vectors: the squares summed
    x, y, z, one square root, three divisions; w passes through."""
    d = np.asarray(directions, dtype=F).copy()
    x = d[:, :3]
    length = np.sqrt(((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(F) + x[:, 2] * x[:, 2]).astype(F)).astype(F)
    d[:, :3] = (x / length[:, None]).astype(F)
    return d
