"""numpy restatement of the three Philox uses of a batch's device loop (csrc/batch_loop.h, include/rfsgpu.h [batch]):
the two Box-Muller blocks of rfsgpu_batch_propagate_async and the resampling draw of rfsgpu_batch_resample_async.
Philox4x32-10: Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11); pinned to the Random123
known-answer vectors in tests/test_batch_device_loop.py."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
U64 = np.uint64


def philox4x32_10(ctr, key):
    c = [np.asarray(x, dtype=U64) for x in ctr]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0 = U64(M0) * c[0]
        p1 = U64(M1) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ U64(k0), p1 & U64(MASK), (p0 >> U64(32)) ^ c[3] ^ U64(k1), p0 & U64(MASK)]
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c


def u01_open_low(a, b):
    """motion.h philox_u01: 53 bits -> (0, 1]."""
    m = ((a << U64(32)) | b) >> U64(11)
    return (m.astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)


def _block(n, block, seed, call):
    i = np.arange(n, dtype=U64)
    z = np.zeros(n, dtype=U64)
    return philox4x32_10([i, z + U64(block), z + U64(call & MASK), z + U64(call >> 32)], (seed & MASK, seed >> 32))


def propagation_deviates(n, seed, call):
    """g [n, 3]: block 0 gives g_x = rad cos, g_y = rad sin; block 1's rad cos gives g_theta."""
    r = _block(n, 0, seed, call)
    rad, ang = np.sqrt(-2.0 * np.log(u01_open_low(r[0], r[1]))), 2.0 * np.pi * u01_open_low(r[2], r[3])
    g = np.empty((n, 3))
    g[:, 0], g[:, 1] = rad * np.cos(ang), rad * np.sin(ang)
    r = _block(n, 1, seed, call)
    rad, ang = np.sqrt(-2.0 * np.log(u01_open_low(r[0], r[1]))), 2.0 * np.pi * u01_open_low(r[2], r[3])
    g[:, 2] = rad * np.cos(ang)
    return g


def resample_draw_bits(seed, call):
    """The 53 bits of block (0, 2, call lo, call hi) under the filter's key."""
    r = philox4x32_10([np.array([0], dtype=U64), np.array([2], dtype=U64), np.array([call & MASK], dtype=U64), np.array([call >> 32], dtype=U64)],
                      (seed & MASK, seed >> 32))
    return (int(r[0][0]) << 32 | int(r[1][0])) >> 11


def resample_draw(seed, call):
    """u in [0, 1)."""
    return resample_draw_bits(seed, call) * (1.0 / 9007199254740992.0)


def odometry_step(x, u):
    """MotionModel_Odometry2d::step (reference src/ProcessModel_Odometry2D.cpp:40-90), x [n, 3], u [3]."""
    th = x[:, 2]
    ct, st = np.cos(th), np.sin(th)
    out = np.empty_like(x)
    out[:, 0] = x[:, 0] + (ct * u[0] - st * u[1])
    out[:, 1] = x[:, 1] + (st * u[0] + ct * u[1])
    cd, sd = np.cos(u[2]), np.sin(u[2])
    out[:, 2] = np.arctan2(cd * st + sd * ct, cd * ct - sd * st)
    return out


def propagate(x, u, var, seed, call):
    """Particle i of a filter: odometry_step(pose, u) + sqrt(var) * g_i."""
    return odometry_step(x, u) + np.sqrt(np.asarray(var, dtype=np.float64)) * propagation_deviates(x.shape[0], seed, call)
