"""kf_ingest / kf_quat_to_euler at the places and stream edges where they could go wrong, against
oracle/ref_ingest.py on the fixed inputs of tests/ingest_cases.py — needs an MI355X.

test_gpu_ingest.py holds the ingest kernels to the reference's goldens: one synthetic log in one
UTM zone.  Here the projection runs over every zone, letter band, exception box and hemisphere,
kf_quat_to_euler through the raw ABI with a padded leading dimension and at its clamp threshold,
and the merge over its edges (GPS only, no fix kept, ties, signed zeros, the bias kernel's
32-row unroll, the 256-thread block edge, padded leading dimensions, NULL outputs, a caller's
biases, non-finite times).  test_ingest_cases_cpu.py shows that the inputs reach all that.

Tolerances, each stated where it comes from:
* zone number and letter (None <-> 0), altitude, time (bit for bit, the sign of zero included),
  merged order, etype, src, the counts, first_valid_index, origin_row, the biases and
  w - bias / a - bias are exact: the same IEEE operations in the same order.
* Easting / northing offsets against the oracle's e - e0, n - n0, and utm_origin against
  (e0, n0): 1e-7 m, the project's figure for device against host libm (test_gpu_ingest.py's
  docstring: sin/cos/pow differ in the last ulp).  An ulp of a 1e7 m northing is 1.9e-9 m; the
  float64 oracle itself is within 2e-8 m of the same formulas in np.longdouble on these points
  (test_ingest_cases_cpu.py), so the tolerance keeps a factor of 5 over the referee's rounding.
* Euler angles: 1e-13 rad (the same docstring: atan2/asin against the host libm).  Where the
  oracle takes the clamp branch the pitch is +-pi/2 bit for bit; the NaN pattern is the oracle's.
  The threshold family (0, +-h, 0, h), h = 0.7071067811865476, has cosr_cosp = 1 - 2(x*x + y*y) =
  -2.2e-16 and so roll = yaw = pi, held to the same 1e-13.  Its products with zero are exact, so
  it reads the same with or without FMA contraction (test_ingest_cases_cpu.py computes both);
  what pins "the reference's order with contraction off" are the contraction witnesses: six
  quaternions 1e-8 rad from gimbal lock whose sinp = 2(w*y - z*x) is >= 1 as two rounded products
  (the clamp, pitch = pi/2 bit for bit) and 1 - 1.1e-16 in either fused form (asin, 1.5e-8 rad
  lower): they fail by 1.5e-8 rad if the pragma or a build flag is lost.
* A kept fix or an IMU row with a NaN or +-inf time: KF_EINVAL naming the sensor and the lowest
  such row; a dropped fix's time is never looked at.

Each test prints its worst differences (pytest -s); profiles/ingest_edges/ingest_edges.log keeps one run.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ingest_cases as ic
from kfmi import KFError, _lib, ingest

pytestmark = pytest.mark.gpu

UTM_TOL = 1e-7      # metres
ANGLE_TOL = 1e-13   # radians


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def raw_ingest(gps, imu, with_altitude=True, bias=None, pad=0, null_outputs=False):
    """kf_ingest through the raw ABI: leading dimensions n + pad (the padding NaN), outputs
    poisoned first; returns the written rows, the info struct's fields and the untouched tails."""
    ng, ni = gps.shape[1], imu.shape[1]
    g, m = _dev(ic.padded(gps, pad)), _dev(ic.padded(imu, pad))
    cap = ng + ni + 3
    etype = torch.full((cap,), 0xEE, dtype=torch.uint8, device='cuda')
    t = torch.full((cap,), float('nan'), dtype=torch.float64, device='cuda')
    payload = torch.full((cap, 9), float('nan'), dtype=torch.float64, device='cuda')
    src = torch.full((cap,), -7, dtype=torch.int32, device='cuda')
    zn = torch.full((cap,), -7, dtype=torch.int8, device='cuda')
    zl = torch.full((cap,), 0xEE, dtype=torch.uint8, device='cuda')
    info = _lib.kf_ingest_info()
    b = None if bias is None else np.ascontiguousarray(np.concatenate([bias[0], bias[1]]), dtype=np.float64)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    opt = (lambda x: None) if null_outputs else p
    _lib.check(_lib.lib().kf_ingest(p(g) if ng else None, ng, ng + pad, p(m) if ni else None, ni, ni + pad,
                                    _lib.KF_INGEST_GPS_ALTITUDE if with_altitude else 0,
                                    None if b is None else b.ctypes.data_as(ctypes.c_void_p),
                                    p(etype), p(t), p(payload), opt(src), opt(zn), opt(zl), ctypes.byref(info),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    n = int(info.n_events)
    out = dict(etype=etype, t=t, payload=payload, src=src, zone_number=zn, zone_letter=zl)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    # nothing past the n_events rows is written
    assert (out['etype'][n:] == 0xEE).all() and np.isnan(out['t'][n:]).all() and np.isnan(out['payload'][n:]).all()
    assert (out['src'][n:] == -7).all() and (out['zone_number'][n:] == -7).all() and (out['zone_letter'][n:] == 0xEE).all()
    if null_outputs:
        assert (out['src'] == -7).all() and (out['zone_number'] == -7).all() and (out['zone_letter'] == 0xEE).all()
    out = {k: v[:n] for k, v in out.items()}
    out.update(n_events=n, n_fixes=int(info.n_fixes), n_imu=int(info.n_imu),
               first_valid_index=int(info.first_valid_index), origin_row=int(info.origin_row),
               gyro_bias=np.array(info.gyro_bias[:]), accel_bias=np.array(info.accel_bias[:]),
               utm_origin=np.array(info.utm_origin[:]))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare_stream(out, ref, label, side_outputs=True):
    """The written stream against ic.reference's arrays: everything exact but the UTM offsets
    (UTM_TOL) and the Euler angles (ANGLE_TOL).  Returns (worst offset, worst angle)."""
    np.testing.assert_array_equal(out['etype'], ref['etype'], err_msg=label)
    np.testing.assert_array_equal(_bits(out['t']), _bits(ref['t']), err_msg=label)     # the sign of zero too
    if side_outputs:
        np.testing.assert_array_equal(out['src'], ref['src'], err_msg=label)
        np.testing.assert_array_equal(out['zone_number'], ref['zone_number'], err_msg=label)
        np.testing.assert_array_equal(out['zone_letter'], ref['zone_letter'], err_msg=label)
    fix, imu = ref['etype'] == ic.GPS, ref['etype'] == ic.IMU
    pf, rf = out['payload'][fix], ref['payload'][fix]
    worst_m = float(np.max(np.abs(pf[:, :2] - rf[:, :2]))) if fix.any() else 0.0
    assert not np.isnan(pf[:, :2]).any(), label
    np.testing.assert_array_equal(pf[:, 2], rf[:, 2], err_msg=label)                   # altitude, NaN where it is missing
    assert (_bits(pf[:, 3:]) == 0).all(), label
    pi, ri = out['payload'][imu], ref['payload'][imu]
    np.testing.assert_array_equal(np.isnan(pi[:, :3]), np.isnan(ri[:, :3]), err_msg=label)
    d = np.abs(pi[:, :3] - ri[:, :3])
    worst_rad = float(np.nanmax(d)) if d.size and not np.isnan(d).all() else 0.0
    np.testing.assert_array_equal(pi[:, 3:], ri[:, 3:], err_msg=label)                 # w - bias, a - bias
    assert worst_m <= UTM_TOL and worst_rad <= ANGLE_TOL, (label, worst_m, worst_rad)
    return worst_m, worst_rad


def compare_info(out, ref, label):
    assert out['n_events'] == len(ref['t']) and out['n_fixes'] == ref['n_fixes'] and out['n_imu'] == ref['n_imu'], label
    assert out['first_valid_index'] == ref['first_valid_index'] and out['origin_row'] == ref['origin_row'], label
    np.testing.assert_array_equal(out['gyro_bias'], ref['gyro_bias'], err_msg=label)   # NaN for an empty slice
    np.testing.assert_array_equal(out['accel_bias'], ref['accel_bias'], err_msg=label)
    worst = float(np.max(np.abs(out['utm_origin'] - ref['utm_origin'])))
    assert worst <= UTM_TOL, (label, worst)
    if ref['n_fixes'] == 0:
        assert out['utm_origin'].tolist() == [0.0, 0.0], label
    return worst


# --------------------------------------------------------------------------------------
# projection
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _projection_inputs(name, with_imu):
    gps = ic.grid_case() if name == 'grid' else ic.track_case(name)
    imu = ic.few_imu_rows(name, 0.5, gps.shape[1] - 1.5) if with_imu else np.zeros((11, 0))
    return gps, imu, ic.reference(gps, imu)


@pytest.mark.parametrize('with_imu', [False, True], ids=['no_imu', 'few_imu'])
@pytest.mark.parametrize('name', ('grid',) + ic.TRACKS)
def test_projection_worldwide(name, with_imu):
    gps, imu, ref = _projection_inputs(name, with_imu)
    s = ingest.ingest_arrays(gps, imu)
    out = dict(s.host())
    label = f'{name}/{"few_imu" if with_imu else "no_imu"}'
    worst_m, _ = compare_stream(out, ref, label)
    fix = ref['etype'] == ic.GPS
    de = float(np.max(np.abs(out['payload'][fix, 0] - ref['payload'][fix, 0])))
    dn = float(np.max(np.abs(out['payload'][fix, 1] - ref['payload'][fix, 1])))
    do = float(np.max(np.abs(s.utm_origin - ref['utm_origin'])))
    print(f'ingest-edges | projection | {label} | {int(fix.sum())} fixes | easting {de:.3e} m | northing {dn:.3e} m | '
          f'utm_origin {do:.3e} m | tolerance {UTM_TOL:.0e} m')
    assert do <= UTM_TOL
    assert s.n_fixes == ref['n_fixes'] == gps.shape[1] and s.n_imu == imu.shape[1] and len(s) == len(ref['t'])
    assert s.first_valid_index == 0 and np.isnan(s.gyro_bias).all() and np.isnan(s.accel_bias).all()
    # every fix of these cases is kept, in row order: zone and letter against the oracle's projection of the row
    e, n, zn, zl = ic.project(gps)
    np.testing.assert_array_equal(out['zone_number'][fix], zn)
    np.testing.assert_array_equal(out['zone_letter'][fix], zl)
    if name == 'grid':
        assert (out['zone_letter'][fix][-len(ic.NO_LETTER_POINTS):] == 0).all()       # None -> 0 on the device


# --------------------------------------------------------------------------------------
# kf_quat_to_euler
# --------------------------------------------------------------------------------------
def raw_euler(q, pad):
    n = q.shape[1]
    qd = _dev(ic.padded(q, pad))
    out = torch.full((3, n), 12345.0, dtype=torch.float64, device='cuda')
    _lib.check(_lib.lib().kf_quat_to_euler(n, ctypes.c_void_p(qd.data_ptr()), n + pad, ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('pad', [0, 5], ids=['ld_n', 'ld_n_plus_5'])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_quat_to_euler_raw_abi(n, pad):
    q, ref = ic.quaternions()[:, :n], ic.euler_reference()[:, :n]
    got = raw_euler(q, pad)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    d = np.abs(got - ref)
    worst = [float(np.nanmax(d[k])) if not np.isnan(d[k]).all() else 0.0 for k in range(3)]
    print(f'ingest-edges | kf_quat_to_euler | n {n} ld {n + pad} | roll {worst[0]:.3e} rad | pitch {worst[1]:.3e} rad | '
          f'yaw {worst[2]:.3e} rad | tolerance {ANGLE_TOL:.0e} rad')
    assert max(worst) <= ANGLE_TOL, worst
    clamp = np.abs(ic.sinp(q)) >= 1
    np.testing.assert_array_equal(_bits(got[1, clamp]), _bits(ref[1, clamp]))          # +-pi/2 exactly
    assert clamp[:min(n, 2)].all() and set(np.abs(ref[1, clamp]).tolist()) == {np.pi / 2}
    # the threshold family: roll = yaw = pi from cosr_cosp = cosy_cosp = -2.2e-16
    k = min(n, 4)
    assert np.max(np.abs(got[[0, 2], :k] - ref[[0, 2], :k])) <= ANGLE_TOL
    assert abs(got[0, 0] - np.pi) <= ANGLE_TOL and abs(got[2, 0] - np.pi) <= ANGLE_TOL
    # the contraction check: the witnesses clamp only with both products of sinp rounded
    if n >= ic.N_SPECIAL:
        assert clamp[ic.WITNESS_AT].all()
        np.testing.assert_array_equal(_bits(got[1, ic.WITNESS_AT]), _bits(np.full(ic.N_WITNESSES, np.pi / 2)))


def test_quaternions_through_ingest_match_quat_to_euler():
    gps, imu = ic.quaternion_case()
    out = raw_ingest(gps, imu)
    rows = out['etype'] == ic.IMU
    order = np.argsort(out['src'][rows], kind='stable')
    ang = out['payload'][rows][order][:, :3].T
    direct = raw_euler(ic.quaternions(), 0)
    np.testing.assert_array_equal(np.isnan(ang), np.isnan(direct))
    ok = ~np.isnan(direct)
    np.testing.assert_array_equal(_bits(ang[ok]), _bits(direct[ok]))                   # one device function, bit for bit
    ref = ic.reference(gps, imu)
    compare_stream(out, ref, 'quaternion_case')
    compare_info(out, ref, 'quaternion_case')


# --------------------------------------------------------------------------------------
# merge
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ic.merge_names())
def test_merge_edges(name):
    c = ic.merge_case(name)
    for alt in ic.merge_flags(name):
        ref = ic.merge_reference(name, alt)
        label = f'{name}/{"altitude" if alt else "no_altitude"}'
        out = raw_ingest(c['gps'], c['imu'], alt, c['bias'])
        worst_m, worst_rad = compare_stream(out, ref, label)
        worst_o = compare_info(out, ref, label)
        if (name, alt) in ic.CLAIMS:
            assert (out['first_valid_index'], out['origin_row'], out['n_fixes'], out['n_imu']) == ic.CLAIMS[name, alt]
        if c['bias'] is not None:   # the caller's biases: used in the payload (compare_stream) and reported
            np.testing.assert_array_equal(out['gyro_bias'], c['bias'][0])
            np.testing.assert_array_equal(out['accel_bias'], c['bias'][1])
        print(f'ingest-edges | merge | {label} | {out["n_fixes"]} fixes + {out["n_imu"]} IMU | offsets {worst_m:.3e} m | '
              f'utm_origin {worst_o:.3e} m | angles {worst_rad:.3e} rad')


@pytest.mark.parametrize('name', ['M5', 'M8_257_300_kept', 'M8_257_300_dropped'])
def test_merge_padded_leading_dimensions_and_null_outputs(name):
    """M9: ld = n + 7 with NaN in the padding columns gives bit for bit the ld = n stream, and so
    does a call without src / zone_number / zone_letter."""
    c, ref = ic.merge_case(name), ic.merge_reference(name)
    plain = raw_ingest(c['gps'], c['imu'], True, c['bias'])
    for pad, null in ((7, False), (7, True), (0, True)):
        label = f'{name}/ld_n_plus_{pad}{"/null_outputs" if null else ""}'
        out = raw_ingest(c['gps'], c['imu'], True, c['bias'], pad=pad, null_outputs=null)
        compare_stream(out, ref, label, side_outputs=not null)
        compare_info(out, ref, label)
        for k, v in plain.items():
            if null and k in ('src', 'zone_number', 'zone_letter'):
                continue
            np.testing.assert_array_equal(out[k], v, err_msg=f'{label}: {k}')


# --------------------------------------------------------------------------------------
# non-finite times
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ic.NONFINITE))
def test_nonfinite_times(name):
    sensor, at, value, rejected, row = ic.NONFINITE[name]
    gps, imu = ic.nonfinite_case(name)
    assert len(ic.kept_rows(gps)) >= 1
    if not rejected:   # a dropped fix: its time is never looked at
        out = raw_ingest(gps, imu)
        ref = ic.reference(gps, imu)
        compare_stream(out, ref, name)
        compare_info(out, ref, name)
        return
    with pytest.raises(KFError, match=f'{sensor.upper()} row {row} ') as e:
        raw_ingest(gps, imu)
    assert e.value.code == _lib.KF_EINVAL and 'not finite' in str(e.value)
    # the same handle-free call with the value repaired succeeds afterwards
    c, ref = ic.merge_case('M5'), ic.merge_reference('M5')
    out = raw_ingest(c['gps'], c['imu'])
    compare_stream(out, ref, name + '/repaired')
    compare_info(out, ref, name + '/repaired')
