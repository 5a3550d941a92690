"""The light and the material of the HIP backend (include/ovr_hip.h, ovr_hip_set_light / ovr_hip_set_material) as a numpy model.

Light direction: a world-space vector TOWARDS the light, any length.  The renderer normalises it with the host routine
`normalize` below (float32: dot by two fused multiply-adds, one square root, three divisions).  The interface's two angles,
in degrees, mean

    d = (sin phi * cos theta,  sin phi * sin theta,  cos phi)          evaluated in double, rounded to float per component

- the convention the interactive app's defaults (phi 99.53, theta 112.2) were written in: they lie 0.15 degrees from the
reference's literal vector.  The state starts as that literal; `angles_of` is the inverse.

Shade factor, per shaded sample (n_w the world-space normal, L the unit light, pos the sample's world position, shadow the
shadow march's alpha - 0 when only the gradient is shaded -, I2 = 2 * intensity formed on the host).  IEEE float32, nothing
contracted, in exactly this order; dot(a, b) = fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)):

    cosNL = |dot(L, n_w)|
    d     = (kd * cosNL) * I2
    if ks > 0:   V = normalize(cam_pos - pos)   H = normalize(L + V)   cosNH = |dot(H, n_w)|
                 sp = exp2(shininess * log2(cosNH))  if cosNH >= 2^-126  else 0
                 d = d + (ks * sp) * I2
    shade = ka + d * (1 - shadow)

The reference state (ka 0.5, kd 0.5, ks 0, intensity 1) is the reference's own `0.5f + 0.5f * cosNL * 2.f * (1.f - shadow)`,
operation for operation.  The specular term is two-sided like the diffuse one.  A NaN normal (zero gradient) gives NaN - the
kernels' clamp01 turns the sample's colour into 0.  Finite inputs never give NaN: a sample at the camera or a half vector of
length 0 make cosNH NaN, the comparison fails and sp = 0.  The guard is `cosNH >= 2^-126` (the smallest normal float) and not
`cosNH > 0`: the hardware logarithm (v_log_f32) takes a denormal for 0 and returns -inf, which shininess 0 - the app's slider
reaches it - would turn into 0 * -inf = NaN.  Below 2^-126 the power is 0 for every shininess a float32 product with -126 does
not round to 0, so the select only moves the discontinuity that shininess 0 has at cosNH = 0 anyway.

log2 / exp2 here are the machine-independent pair of the exact-parity build (ovr_hip_device.h det_log2f / det_exp2f): that
build reproduces `shade` bit for bit (tests/test_lighting_gpu.py).  The product evaluates them with v_log_f32 / v_exp_f32 and
normalises with v_rsq_f32; its distance from this model is measured in profiles/r08_lighting.md."""
import numpy as np

F = np.float32
LITERAL_LIGHT = (F(-907.108), F(2205.875), F(-400.0267))  # the reference's light, a vector towards it
REFERENCE_MATERIAL = (0.5, 0.5, 0.0, 0.0)                  # ambient, diffuse, specular, shininess; intensity 1
APP_DEFAULT_ANGLES = (99.53, 112.2)                        # phi, theta of the interactive app's sliders
APP_DEFAULT_MATERIAL = (0.6, 0.9, 0.4, 40.0)
FLT_MIN = F(1.17549435e-38)


def fma(a, b, c):
    """fused multiply-add of float32 arrays, correctly rounded: the product of two float32 is exact in double; the sum is
    rounded to odd in double (TwoSum gives the rounding's direction), so that the second rounding to float32 cannot go wrong"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)  # the neighbour of s on the side of the exact sum
        return s.astype(F)


def dot(a, b):
    return fma(a[..., 0], b[..., 0], fma(a[..., 1], b[..., 1], np.asarray(a[..., 2], F) * np.asarray(b[..., 2], F)))


def normalize(v):
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.sqrt(dot(v, v))
        return ((v * F(1)) / l[..., None]).astype(F)


def direction_from_angles(phi, theta):
    """degrees -> the raw float32 vector handed to ovr_hip_set_light"""
    p, t = np.deg2rad(np.float64(phi)), np.deg2rad(np.float64(theta))
    return np.array([np.sin(p) * np.cos(t), np.sin(p) * np.sin(t), np.cos(p)], np.float64).astype(F)


def angles_of(v):
    """(phi, theta) in degrees of a vector of any length"""
    v = np.asarray(v, np.float64)
    return float(np.rad2deg(np.arccos(v[2] / np.linalg.norm(v)))), float(np.rad2deg(np.arctan2(v[1], v[0])))


def _horner(coeffs, x):
    p = np.full(x.shape, F(coeffs[0]), F)
    for c in coeffs[1:]:
        p = fma(p, x, F(c))
    return p


_LOG2 = [float.fromhex(h) for h in ("-0x1.b8f078p-4", "0x1.7aec18p-3", "-0x1.881ca4p-3", "0x1.a37bc2p-3", "-0x1.eab168p-3", "0x1.277a9ap-2",
                                    "-0x1.715a9p-2", "0x1.ec70a8p-2", "-0x1.71547p-1", "0x1.715476p+0")]
_EXP2 = [float.fromhex(h) for h in ("0x1.00c0e4p-16", "0x1.446c7ap-13", "0x1.5d8776p-10", "0x1.3b29d8p-7", "0x1.c6b08ep-5", "0x1.ebfbep-3",
                                    "0x1.62e43p-1", "0x1p+0")]


def det_log2(x):
    """the exact-parity build's log2 for NORMAL positive finite float32 (all the shade factor hands it)"""
    x = np.asarray(x, F)
    ix = x.view(np.uint32)
    e = (ix >> 23).astype(np.int32) - 127
    m = ((ix & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(F)
    big = m > F(float.fromhex("0x1.6a09e6p+0"))
    m = np.where(big, m * F(0.5), m).astype(F)
    e = e + big
    f = (m - F(1)).astype(F)
    return fma(f, _horner(_LOG2, f), e.astype(F))


def det_exp2(m):
    m = np.asarray(m, F)
    with np.errstate(invalid="ignore", over="ignore"):
        mm = np.where(np.isfinite(m) & (m < 128) & (m >= -126), m, F(0)).astype(F)
        n = np.floor((mm + F(0.5)).astype(F))
        r = (mm - n).astype(F)
        p = _horner(_EXP2, r)
        i = n.astype(np.int32)
        h = np.where(i < 0, -((-i) // 2), i // 2)  # C division truncates
        s = ((p * ((h + 127).astype(np.uint32) << 23).view(F)).astype(F) * ((i - h + 127).astype(np.uint32) << 23).view(F)).astype(F)
        s = np.where(s < FLT_MIN, F(0), s)
        s = np.where(m >= 128, F(np.inf), np.where(m < -126, F(0), s))
        return np.where(np.isnan(m), m, s).astype(F)


def specular_power(cosNH, shininess):
    cosNH = np.asarray(cosNH, F)
    ok = cosNH >= FLT_MIN  # false for NaN
    x = np.where(ok, cosNH, F(1)).astype(F)
    return np.where(ok, det_exp2((F(shininess) * det_log2(x)).astype(F)), F(0)).astype(F)


def shade(normal_w, pos, shadow, light, cam_pos, ambient=0.5, diffuse=0.5, specular=0.0, shininess=0.0, intensity=1.0, view=None):
    """the shade factor of n samples: normal_w (n, 3), pos (n, 3), shadow (n,); light = the UNIT direction (normalize(raw)).  view: the view vector of every
    sample, used as given (the orthographic camera's -dir, camera.py); None = normalize(cam_pos - pos), the perspective camera's"""
    n_w, pos, shadow = np.asarray(normal_w, F), np.asarray(pos, F), np.asarray(shadow, F)
    L, cam = np.asarray(light, F), np.asarray(cam_pos, F)
    ka, kd, ks, i2 = np.asarray(ambient, F), F(diffuse), F(specular), F(2) * F(intensity)   # (ambient: a scalar, or one per sample - isosurface.py's occlusion)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cosNL = np.abs(dot(np.broadcast_to(L, n_w.shape), n_w))
        d = ((kd * cosNL).astype(F) * i2).astype(F)
        if ks > 0:
            V = normalize((cam - pos).astype(F)) if view is None else np.broadcast_to(np.asarray(view, F), n_w.shape)
            H = normalize((L + V).astype(F))
            cosNH = np.abs(dot(H, n_w))
            sp = specular_power(cosNH, shininess)
            d = (d + ((ks * sp).astype(F) * i2).astype(F)).astype(F)
        return (ka + (d * (F(1) - shadow).astype(F)).astype(F)).astype(F)


def reference_shade(cosNL, shadow):
    """the reference's literal expression, 0.5f + 0.5f * cosNL * 2.f * (1.f - shadow), as C evaluates it"""
    cosNL, shadow = np.asarray(cosNL, F), np.asarray(shadow, F)
    return (F(0.5) + (((F(0.5) * cosNL).astype(F) * F(2)).astype(F) * (F(1) - shadow).astype(F)).astype(F)).astype(F)
