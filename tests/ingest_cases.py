"""The fixed inputs of the ingest edge tests and, cached, what ``oracle/ref_ingest.py`` makes of them.

``test_gpu_ingest_edges.py`` runs ``kf_ingest`` / ``kf_quat_to_euler`` on these inputs;
``test_ingest_cases_cpu.py`` asserts, for the very same inputs, that they reach the zones, letters,
branches, ties and drops they are named for — so nobody loosens the GPU test by changing a seed
or a shape here.  Every random draw is seeded from the case's name.

The oracle is fed string rows made with ``repr()`` and ``'nan'`` for a missing field, the way the
reference reads its CSV files (``rows``).

Projection grid (``grid_case``): the cross product of
  latitudes   every band edge -80, -72, ..., 72 and 84; 0 and +-1e-9; 56, 64, 72 and the double
              just below each;
  longitudes  every multiple of 6 in [-180, 180) and the double just below it, each zone's centre
              and its east edge minus 1e-3, 180.0 itself (zone 61), the exception edges 0, 3, 9,
              12, 21, 33, 42 and the double just below each;
then 2,000 random points, then one point at latitude 85 and one at -80.5 (no zone letter).
Tracks (``track_case``): across a zone boundary, across the equator, inside the Norway box and
inside the Svalbard box.  Offsets are relative to the first kept fix, as the reference computes.

Quaternions (``quaternions``): the threshold family, the axis and zero quaternions, one NaN per
component, the contraction witnesses (``contraction_witnesses``), then random unit quaternions and
the same scaled to norm 0.5 and 2.

Merge cases (``merge_case``; CLAIMS holds the info fields stated by hand):
  M1  GPS only;                          M2  row 0 with a latitude but no longitude;
  M3  every fix dropped, one latitude;   M4  altitude-only gaps, under both flags;
  M5  ties of every kind, IMU rows locally out of order, a fix before and one after all IMU rows;
  M6  negative times, a 0.0 / -0.0 tie across the sensors;
  M7_f<k>  first_valid_index k in 1, 31, 32, 33, 95 of 100 IMU rows, 120 (above them), M7_bias;
  M8_<n_gps>_<n_imu>_<kept|dropped>  the 256-thread block edge, scattered drops, the last GPS row
      kept or dropped.
M9 is M5 and M8_257_300_* run with padded leading dimensions (``padded``) and NULL outputs; that is
the GPU test's doing, the inputs are these.
"""
import functools
import math
import warnings
import zlib
from fractions import Fraction

import numpy as np

from oracle import ref_ingest as R

H = 0.7071067811865476
H_BELOW = float(np.nextafter(H, 0.0))
GPS, IMU = 0, 1


def _rng(*parts):
    return np.random.default_rng(zlib.crc32('/'.join(map(str, parts)).encode()))


def rows(cols):
    """[k, n] columns -> the n string rows csv.reader would give: repr() per field, 'nan' for NaN."""
    a = np.asarray(cols, dtype=np.float64)
    return [['nan' if np.isnan(v) else repr(float(v)) for v in a[:, i]] for i in range(a.shape[1])]


def padded(cols, pad):
    """The columns with ``pad`` more NaN entries each: a leading dimension above the row count."""
    a = np.asarray(cols, dtype=np.float64)
    out = np.full((a.shape[0], a.shape[1] + pad), np.nan)
    out[:, :a.shape[1]] = a
    return out


# --------------------------------------------------------------------------------------
# projection
# --------------------------------------------------------------------------------------
BAND_EDGES = [float(v) for v in range(-80, 73, 8)] + [84.0]
EXCEPTION_EDGES = [0.0, 3.0, 9.0, 12.0, 21.0, 33.0, 42.0]
NO_LETTER_POINTS = [(85.0, 10.0), (-80.5, -70.0)]
N_RANDOM = 2000


def grid_latitudes():
    box = [56.0, 64.0, 72.0]
    return np.unique(BAND_EDGES + [0.0, 1e-9, -1e-9] + box + [float(np.nextafter(v, -np.inf)) for v in box])


def grid_longitudes():
    six = np.arange(-180.0, 180.0, 6.0)
    exc = np.array(EXCEPTION_EDGES)
    return np.unique(np.concatenate([six, np.nextafter(six, -np.inf), six + 3.0, six + 6.0 - 1e-3, [180.0],
                                     exc, np.nextafter(exc, -np.inf)]))


def _fixes(name, lat, lon):
    """gps [4, n] for the points, every one a kept fix: time = its index, a random altitude."""
    n = len(lat)
    return np.stack([np.arange(n, dtype=np.float64), lat, lon, _rng('altitude', name).normal(100.0, 50.0, n)])


@functools.lru_cache(maxsize=None)
def grid_case():
    la, lo = np.meshgrid(grid_latitudes(), grid_longitudes(), indexing='ij')
    rng = _rng('projection grid')
    lat = np.concatenate([la.ravel(), rng.uniform(-80.0, 84.0, N_RANDOM), [p[0] for p in NO_LETTER_POINTS]])
    lon = np.concatenate([lo.ravel(), rng.uniform(-180.0, 180.0, N_RANDOM), [p[1] for p in NO_LETTER_POINTS]])
    return _fixes('grid', lat, lon)


TRACKS = ('zone_boundary', 'equator', 'norway', 'svalbard')
TRACK_POINTS = 96


@functools.lru_cache(maxsize=None)
def track_case(name):
    s = np.linspace(0.0, 1.0, TRACK_POINTS)
    w = _rng('track', name).normal(0.0, 1e-5, (2, TRACK_POINTS))
    lat, lon = {'zone_boundary': (45.0 + 0.01 * s, 5.99 + 0.02 * s),        # zone 31 -> 32 at longitude 6
                'equator': (-0.001 + 0.002 * s, -60.5 + 0.01 * s),          # northing offset 10,000,000 -> 0
                'norway': (56.5 + 7.0 * s, 3.2 + 8.6 * s),                  # 56 <= lat < 64, 3 <= lon < 12
                'svalbard': (72.5 + 11.0 * s, 0.5 + 41.0 * s)}[name]        # 72 <= lat <= 84, 0 <= lon < 42
    return _fixes(name, lat + w[0], lon + w[1])


def few_imu_rows(name, t_lo, t_hi, n=5):
    """A few IMU rows with times inside [t_lo, t_hi], for the projection runs 'with a few'."""
    rng = _rng('few imu', name)
    imu = rng.normal(size=(11, n))
    imu[0] = np.sort(rng.uniform(t_lo, t_hi, n))
    return imu


def project(gps):
    """The oracle's utm_from_latlon on every row: (easting, northing, zone number, letter or 0)."""
    out = [R.utm_from_latlon(float(la), float(lo)) for la, lo in zip(gps[1], gps[2])]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([ord(o[3]) if o[3] else 0 for o in out]))


def project_longdouble(lat, lon, zone):
    """oracle/ref_ingest.utm_from_latlon's formulas in np.longdouble (the zone given): the
    yardstick for the float64 oracle's own rounding."""
    L = np.longdouble
    e = L(R.E)
    e2, e3, ep2 = e * e, e * e * e, e / (1 - e)
    m1 = 1 - e / 4 - 3 * e2 / 64 - 5 * e3 / 256
    m2 = 3 * e / 8 + 3 * e2 / 32 + 45 * e3 / 1024
    m3 = 15 * e2 / 256 + 45 * e3 / 1024
    m4 = 35 * e3 / 3072
    rad = L(np.pi) / 180
    lat_rad, lon_rad = np.asarray(lat, L) * rad, np.asarray(lon, L) * rad
    s, c_ = np.sin(lat_rad), np.cos(lat_rad)
    t = s / c_
    t2, t4 = t * t, t * t * t * t
    central = ((np.asarray(zone, L) - 1) * 6 - 180 + 3) * rad
    n = L(R.R_EARTH) / np.sqrt(1 - e * s ** 2)
    c = ep2 * c_ ** 2
    a = c_ * (lon_rad - central)
    m = L(R.R_EARTH) * (m1 * lat_rad - m2 * np.sin(2 * lat_rad) + m3 * np.sin(4 * lat_rad) - m4 * np.sin(6 * lat_rad))
    k0 = L(R.K0)
    east = k0 * n * (a + a ** 3 / 6 * (1 - t2 + c) + a ** 5 / 120 * (5 - 18 * t2 + t4 + 72 * c - 58 * ep2)) + 500000
    north = k0 * (m + n * t * (a ** 2 / 2 + a ** 4 / 24 * (5 - t2 + 9 * c + 4 * c ** 2)
                               + a ** 6 / 720 * (61 - 58 * t2 + t4 + 600 * c - 330 * ep2)))
    return east, np.where(np.asarray(lat) < 0, north + 10000000, north)


# --------------------------------------------------------------------------------------
# quaternions
# --------------------------------------------------------------------------------------
WITNESS_AT = slice(15, 21)    # after the threshold family (4), six axis, the zero and four NaN quaternions
N_SPECIAL = 21
THRESHOLD_FAMILY = [(0.0, H, 0.0, H), (0.0, -H, 0.0, H),      # sinp = +-1.0000000000000002: the clamp
                    (0.0, H, 0.0, H_BELOW),                   # sinp exactly 1.0
                    (0.0, H_BELOW, 0.0, H_BELOW)]             # sinp = 0.9999999999999998: asin
N_QUATERNIONS = 1000
N_WITNESSES = 6


def fma(a, b, c):
    """a * b + c rounded once, as a fused multiply-add gives it."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def sinp_contracted(x, y, z, w):
    """The two ways a compiler may contract sinp = 2 * (w * y - z * x)."""
    return 2 * fma(w, y, -(z * x)), 2 * fma(-z, x, w * y)


@functools.lru_cache(maxsize=None)
def contraction_witnesses():
    """Quaternions 1e-8 rad from gimbal lock, every component far from zero, whose sinp in the
    reference's order (two products, each rounded, then the difference) is >= 1 - the clamp,
    pitch = pi/2 exactly - while either fused form gives 1 - 1.1e-16, the asin branch and a pitch
    1.5e-8 rad lower.  The threshold family cannot tell: its products with zero are exact, so fused
    and unfused agree there."""
    rng = _rng('contraction witnesses')
    out = []
    while len(out) < N_WITNESSES:
        r, yaw = rng.uniform(-3.0, 3.0, 2)
        p = math.pi / 2 - rng.uniform(0.0, 3e-8)
        cr, sr, cp, sp, cy, sy = (math.cos(r / 2), math.sin(r / 2), math.cos(p / 2), math.sin(p / 2),
                                  math.cos(yaw / 2), math.sin(yaw / 2))
        w, x = cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy
        y, z = cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy
        if min(abs(x), abs(y), abs(z), abs(w)) > 0.05 and 2 * (w * y - z * x) >= 1 and max(sinp_contracted(x, y, z, w)) < 1:
            out.append((x, y, z, w))
    return out


@functools.lru_cache(maxsize=None)
def quaternions():
    """[4, 1000] (x, y, z, w): the special ones first, so every prefix of 255 or more has them all."""
    nan = float('nan')
    special = list(THRESHOLD_FAMILY)
    special += [(1.0, 0, 0, 0), (0, 1.0, 0, 0), (0, 0, 1.0, 0), (0, 0, 0, 1.0), (-1.0, 0, 0, 0), (0, 0, 0, -1.0),
                (0.0, 0.0, 0.0, 0.0)]
    special += [(nan, 0.1, 0.2, 0.9), (0.1, nan, 0.2, 0.9), (0.1, 0.2, nan, 0.9), (0.1, 0.2, 0.9, nan)]
    special += contraction_witnesses()
    k = (N_QUATERNIONS - len(special)) // 3
    u = _rng('quaternions').normal(size=(4, k))
    u /= np.linalg.norm(u, axis=0)
    q = np.concatenate([np.array(special, dtype=np.float64).T, u, 0.5 * u, 2.0 * u], axis=1)
    fill = _rng('quaternions', 'fill').normal(size=(4, N_QUATERNIONS - q.shape[1]))
    return np.concatenate([q, fill / np.linalg.norm(fill, axis=0)], axis=1)


def sinp(q):
    """The reference's sinp for every column, as its float64 arithmetic gives it."""
    return np.array([2 * (float(w) * float(y) - float(z) * float(x)) for x, y, z, w in q.T])


def cosr_cosp(q):
    return np.array([1 - 2 * (float(x) * float(x) + float(y) * float(y)) for x, y, z, w in q.T])


@functools.lru_cache(maxsize=None)
def euler_reference():
    """[3, 1000] (roll, pitch, yaw) of quaternions() by the oracle's quaternion_to_euler."""
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return np.array([R.quaternion_to_euler(*(float(v) for v in col)) for col in quaternions().T], dtype=np.float64).T


@functools.lru_cache(maxsize=None)
def quaternion_case():
    """The quaternion set as the IMU rows of a kf_ingest call: (gps [4, 3], imu [11, 1000])."""
    rng = _rng('quaternion case')
    q = quaternions()
    imu = rng.normal(size=(11, q.shape[1]))
    imu[0] = 0.005 * np.arange(q.shape[1])
    imu[1:5] = q
    gps = np.array([[-1.0, 2.0, 9.0], [40.0, 40.0001, 40.0002], [-75.0, -75.0001, -75.0002], [1.0, 2.0, 3.0]])
    return gps, imu


# --------------------------------------------------------------------------------------
# merge cases
# --------------------------------------------------------------------------------------
def _sensors(name, n_gps, n_imu):
    """Random rows: fixes within ~100 m of (40, -75), IMU rows with unit quaternions; the times
    are the case's to set."""
    rng = _rng('merge', name)
    gps = np.stack([np.zeros(n_gps), 40.0 + rng.normal(0, 1e-3, n_gps), -75.0 + rng.normal(0, 1e-3, n_gps),
                    rng.normal(10.0, 1.0, n_gps)])
    imu = rng.normal(size=(11, n_imu))
    imu[1:5] /= np.maximum(np.linalg.norm(imu[1:5], axis=0), 1e-300)
    return rng, gps, imu


M5_GPS_T = [-1.0, -2.0, 0.5, 2.0, 2.0, 2.25, 3.0, 5.0, 5.0, 7.0, 100.0]   # rows 0, 1 and 5 are dropped
M5_IMU_T = [1.0, 1.0, 2.5, 3.0, 4.5, 4.25, 5.0, 5.0, 6.0, 7.0, 7.0, 8.0]
M6_GPS_T = [-5.5, -0.0, 0.0, 3.0]
M6_IMU_T = [-7.0, -5.5, 0.0, -0.0, 1.0]
M7_COUNTS = (1, 31, 32, 33, 95, 120)
M7_N_IMU = 100
M8_N_GPS = (255, 256, 257)
M8_N_IMU = (0, 1, 300)

# info fields stated by hand, per (case, with_altitude): first_valid_index, origin_row, n_fixes, n_imu
CLAIMS = {('M1', True): (2, 2, 37, 0), ('M2', True): (0, 3, 9, 20), ('M3', True): (2, -1, 0, 10),
          ('M4', True): (1, 2, 11, 24), ('M4', False): (1, 1, 15, 24), ('M5', True): (2, 2, 8, 12),
          ('M6', True): (0, 0, 4, 5), ('M7_f120', True): (120, 120, 4, 100), ('M7_bias', True): (33, 33, 4, 100)}


def merge_names():
    return (['M1', 'M2', 'M3', 'M4', 'M5', 'M6'] + [f'M7_f{k}' for k in M7_COUNTS] + ['M7_bias']
            + [f'M8_{g}_{i}_{last}' for g in M8_N_GPS for i in M8_N_IMU for last in ('kept', 'dropped')])


def merge_flags(name):
    """The with_altitude settings a case runs under."""
    return (True, False) if name == 'M4' else (True,)


@functools.lru_cache(maxsize=None)
def merge_case(name):
    """dict(gps [4, n], imu [11, m], bias: None or (w[3], a[3]))."""
    nan = np.nan
    bias = None
    if name == 'M1':
        rng, gps, imu = _sensors(name, 40, 0)
        gps[0] = 0.1 * np.arange(40)
        gps[1:, :2] = nan
        gps[2, 5] = nan
    elif name == 'M2':
        rng, gps, imu = _sensors(name, 12, 20)
        gps[0] = 0.1 * np.arange(12)
        imu[0] = 0.05 * np.arange(20) + 0.01
        gps[2:, 0] = nan            # row 0: a latitude, no longitude
        gps[1:, 1:3] = nan
    elif name == 'M3':
        rng, gps, imu = _sensors(name, 6, 10)
        gps[0] = 0.1 * np.arange(6)
        imu[0] = 0.05 * np.arange(10) + 0.01
        gps[2] = nan
        gps[1, [0, 1, 3, 4, 5]] = nan
    elif name == 'M4':
        rng, gps, imu = _sensors(name, 16, 24)
        gps[0] = 0.1 * np.arange(16)
        imu[0] = 0.07 * np.arange(24) + 0.01
        gps[1:, 0] = nan
        gps[3, [1, 5, 9, 15]] = nan
    elif name == 'M5':
        rng, gps, imu = _sensors(name, len(M5_GPS_T), len(M5_IMU_T))
        gps[0], imu[0] = M5_GPS_T, M5_IMU_T
        gps[1:, :2] = nan
        gps[1, 5] = nan
    elif name == 'M6':
        rng, gps, imu = _sensors(name, len(M6_GPS_T), len(M6_IMU_T))
        gps[0], imu[0] = M6_GPS_T, M6_IMU_T
    elif name.startswith('M7'):
        k = 33 if name == 'M7_bias' else int(name[4:])
        rng, gps, imu = _sensors(name, k + 4, M7_N_IMU)
        gps[0] = 0.05 * np.arange(k + 4)
        imu[0] = 0.013 * np.arange(M7_N_IMU) + 0.001
        gps[1, :k] = nan            # the latitude alone decides first_valid_index
        if name == 'M7_bias':
            bias = (rng.normal(0, 0.01, 3), rng.normal(0, 0.1, 3))
    elif name.startswith('M8'):
        _, ng, ni, last = name.split('_')
        ng, ni = int(ng), int(ni)
        rng, gps, imu = _sensors(name, ng, ni)
        gps[0] = np.round(rng.uniform(0.0, 10.0, ng), 2)     # out of order, with ties
        imu[0] = np.round(rng.uniform(0.0, 10.0, ni), 2)
        drop = np.nonzero(rng.random(ng) < 0.2)[0]
        gps[rng.integers(1, 4, len(drop)), drop] = nan       # a latitude, a longitude or an altitude
        gps[1:, ng - 1] = gps[1:, ng - 2] = [40.0002, -75.0002, 12.0]
        if last == 'dropped':
            gps[2, ng - 1] = nan
    else:
        raise KeyError(name)
    return dict(gps=gps, imu=imu, bias=bias)


def kept_rows(gps, with_altitude=True):
    """The GPS rows the reference keeps, by NumPy alone (kf_workers.py:310 / hw5_2.py:35)."""
    bad = np.isnan(gps[1]) | np.isnan(gps[2])
    if with_altitude:
        bad |= np.isnan(gps[3])
    return np.nonzero(~bad)[0]


def reference(gps, imu, with_altitude=True, bias=None):
    """The oracle's ingest of the columns, as the arrays kf_ingest writes: dict(etype, t, src,
    payload [N, 9], zone_number, zone_letter (0 for None and for IMU rows), first_valid_index,
    origin_row, n_fixes, n_imu, gyro_bias, accel_bias, utm_origin).  A fix's altitude slot is the
    row's altitude field also where the reference stores none (hw5_2's mode)."""
    g_rows, i_rows = rows(gps), rows(imu)
    utm = R.gps_to_modified_utm(g_rows, with_altitude)
    kept = kept_rows(gps, with_altitude)
    assert len(kept) == len(utm)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')   # the mean of an empty slice, asin(NaN)
        bw, ba, fvi = R.compute_imu_biases(g_rows, i_rows)
        bw, ba = np.broadcast_to(bw, (3,)).copy(), np.broadcast_to(ba, (3,)).copy()
        if bias is not None:
            bw, ba = np.asarray(bias[0], dtype=np.float64), np.asarray(bias[1], dtype=np.float64)
        unb = R.unbias_imu_data(i_rows, bw, ba)
    fix_pos = {id(d): k for k, d in enumerate(utm)}
    imu_pos = {id(e): j for j, e in enumerate(unb)}
    events = R.combine_sensor_data(utm, unb)
    N = len(events)
    out = dict(etype=np.zeros(N, np.uint8), t=np.zeros(N), src=np.zeros(N, np.int32), payload=np.zeros((N, 9)),
               zone_number=np.zeros(N, np.int8), zone_letter=np.zeros(N, np.uint8))
    for i, kind, t, d in events:
        out['t'][i] = t
        if kind == 'GPS':
            k = fix_pos[id(d)]
            out['etype'][i], out['src'][i] = GPS, k
            out['payload'][i, :3] = d['easting'], d['northing'], gps[3, kept[k]]
            out['zone_number'][i] = d['zone_number']
            out['zone_letter'][i] = ord(d['zone_letter']) if d['zone_letter'] else 0
        else:
            out['etype'][i], out['src'][i] = IMU, imu_pos[id(d)]
            out['payload'][i] = [float(v) for v in d[1:10]]
    origin = R.utm_from_latlon(float(gps[1, kept[0]]), float(gps[2, kept[0]]))[:2] if len(kept) else (0.0, 0.0)
    out.update(first_valid_index=fvi, origin_row=int(kept[0]) if len(kept) else -1, n_fixes=len(utm),
               n_imu=imu.shape[1], gyro_bias=bw, accel_bias=ba, utm_origin=np.array(origin))
    return out


@functools.lru_cache(maxsize=None)
def merge_reference(name, with_altitude=True):
    c = merge_case(name)
    return reference(c['gps'], c['imu'], with_altitude, c['bias'])


# --------------------------------------------------------------------------------------
# non-finite times: every case keeps at least one kept fix (M5 has eight)
# --------------------------------------------------------------------------------------
# name -> (sensor, rows, value, rejected, the row the error names)
NONFINITE = {'imu_nan': ('imu', (7, 3), float('nan'), True, 3),
             'imu_plus_inf': ('imu', (4,), float('inf'), True, 4),
             'imu_minus_inf': ('imu', (0, 11), float('-inf'), True, 0),
             'kept_fix_nan': ('gps', (9, 6), float('nan'), True, 6),
             'dropped_fix_nan': ('gps', (0, 5), float('nan'), False, None)}


def nonfinite_case(name):
    """M5 with the time of the named rows replaced: (gps, imu)."""
    sensor, at, value, _, _ = NONFINITE[name]
    c = merge_case('M5')
    gps, imu = c['gps'].copy(), c['imu'].copy()
    (gps if sensor == 'gps' else imu)[0, list(at)] = value
    return gps, imu
