"""The ingest edge cases (tests/ingest_cases.py) do what they claim — on the oracle alone, no GPU.

test_gpu_ingest_edges.py holds kf_ingest and kf_quat_to_euler to oracle/ref_ingest.py on these
inputs; here the same inputs are shown to reach every zone, letter, branch, tie and drop they are
named for, and the float64 oracle's own rounding is measured against the same formulas in
np.longdouble, so the GPU tolerance (1e-7 m) keeps its margin over the referee's error.
"""
import numpy as np
import pytest

import ingest_cases as ic
from oracle import ref_ingest

ORACLE_ROUNDING_CAP = 2e-8   # metres, float64 oracle against np.longdouble: a fifth of the GPU tolerance


def test_grid_reaches_every_zone_letter_and_exception():
    gps = ic.grid_case()
    lat, lon = gps[1], gps[2]
    e, n, zn, zl = ic.project(gps)
    assert set(zn.tolist()) == set(range(1, 62))                    # all 60 zones, and 61 at longitude 180.0
    assert set(zn[lon == 180.0].tolist()) == {61}
    assert {chr(c) for c in zl if c} == set('CDEFGHJKLMNPQRSTUVWX') and len(set('CDEFGHJKLMNPQRSTUVWX')) == 20
    none = zl == 0
    assert sorted(zip(lat[none].tolist(), lon[none].tolist())) == sorted(ic.NO_LETTER_POINTS)
    assert (lat < 0).any() and (lat > 0).any() and (lat == 0).any()
    assert n[(lat < 0) & (lat > -1e-8)].min() > 9.99e6 and n[(lat >= 0) & (lat < 1e-8)].max() < 1   # the offset
    # every band edge, and 84 itself, with its own letter
    for k, edge in enumerate(ic.BAND_EDGES):
        assert {chr(c) for c in zl[lat == edge]} == {'CDEFGHJKLMNPQRSTUVWXX'[k]}, edge
    # the Norway box and its edges
    nor = (lat >= 56) & (lat < 64) & (lon >= 3) & (lon < 12)
    assert nor.any() and set(zn[nor].tolist()) == {32}
    for la, lo, want in [(56.0, 3.0, 32), (np.nextafter(56.0, 0), 3.0, 31), (56.0, np.nextafter(3.0, 0), 31),
                         (np.nextafter(64.0, 0), 3.0, 32), (64.0, 3.0, 31), (56.0, np.nextafter(12.0, 0), 32),
                         (56.0, 12.0, 33), (56.0, 6.0, 32), (56.0, np.nextafter(6.0, 0), 32)]:
        at = (lat == la) & (lon == lo)
        assert at.sum() == 1 and zn[at][0] == want, (la, lo, want, zn[at])
    # the Svalbard box: zones 31, 33, 35, 37 and never 32, 34, 36 from 72 up to and including 84
    sval = (lat >= 72) & (lat <= 84) & (lon >= 0) & (lon < 42)
    assert set(zn[sval].tolist()) == {31, 33, 35, 37}
    for la in (72.0, 84.0):
        # (the double below 0 is outside the box, and -5e-324 + 180 == 180 gives 31 by the plain rule too)
        for lo, want in [(0.0, 31), (np.nextafter(0.0, -1), 31), (np.nextafter(9.0, 0), 31), (9.0, 33),
                         (np.nextafter(21.0, 0), 33), (21.0, 35), (np.nextafter(33.0, 0), 35), (33.0, 37),
                         (np.nextafter(42.0, 0), 37), (42.0, 38)]:
            at = (lat == la) & (lon == lo)
            assert at.sum() == 1 and zn[at][0] == want, (la, lo, want, zn[at])
    below = lat == np.nextafter(72.0, 0)
    assert {32, 34, 36} <= set(zn[below].tolist())
    # both sides of every six-degree edge, and truncation toward zero just below -180.  The double
    # below an edge falls into the zone before it only where lon + 180 does not round back up to
    # the edge (the ulp of lon against the ulp of lon + 180): both kinds are on the grid.
    six = np.arange(-174.0, 180.0, 6.0)
    stays = 0
    for lo in six:
        z = int(round((lo + 180) / 6)) + 1
        lo_b = float(np.nextafter(lo, -np.inf))
        z_b = z if lo_b + 180 == lo + 180 else z - 1
        stays += z_b == z
        assert set(zn[(lon == lo) & (lat == 40.0)].tolist()) == {z}
        assert set(zn[(lon == lo_b) & (lat == 40.0)].tolist()) == {z_b}, lo
    assert 5 <= stays <= len(six) - 5
    assert set(zn[lon == np.nextafter(-180.0, -np.inf)].tolist()) == {1}
    print(f'projection grid: {gps.shape[1]} points, {len(ic.grid_latitudes())} latitudes x '
          f'{len(ic.grid_longitudes())} longitudes + {ic.N_RANDOM} random + {len(ic.NO_LETTER_POINTS)} without a letter')


def test_tracks_cross_what_they_are_named_for():
    for name in ic.TRACKS:
        gps = ic.track_case(name)
        e, n, zn, zl = ic.project(gps)
        if name == 'zone_boundary':
            assert zn[0] == 31 and zn[-1] == 32 and set(zn.tolist()) == {31, 32}
            assert abs(e[-1] - e[0]) > 4e5           # the easting jumps from one zone's east edge to the next's west
        elif name == 'equator':
            assert gps[1, 0] < 0 < gps[1, -1] and n[0] > 9.99e6 and n[-1] < 1e3
            assert {chr(c) for c in zl} == {'M', 'N'}
        elif name == 'norway':
            assert ((gps[1] >= 56) & (gps[1] < 64) & (gps[2] >= 3) & (gps[2] < 12)).all() and set(zn.tolist()) == {32}
            assert (gps[2] < 6).any()                # where the plain rule would say 31
        else:
            assert ((gps[1] >= 72) & (gps[1] <= 84) & (gps[2] >= 0) & (gps[2] < 42)).all()
            assert set(zn.tolist()) == {31, 33, 35, 37}


def test_oracle_rounding_stays_a_fifth_of_the_gpu_tolerance():
    """The float64 oracle against its formulas in np.longdouble, on every grid and track point."""
    assert np.finfo(np.longdouble).eps < 2e-19       # x87 extended precision
    worst_e = worst_n = 0.0
    for gps in [ic.grid_case()] + [ic.track_case(t) for t in ic.TRACKS]:
        e, n, zn, _ = ic.project(gps)
        xe, xn = ic.project_longdouble(gps[1], gps[2], zn)
        worst_e = max(worst_e, float(np.max(np.abs(e - xe))))
        worst_n = max(worst_n, float(np.max(np.abs(n - xn))))
    print(f'oracle rounding against longdouble: easting {worst_e:.3e} m, northing {worst_n:.3e} m '
          f'(cap {ORACLE_ROUNDING_CAP:.0e})')
    assert worst_e <= ORACLE_ROUNDING_CAP and worst_n <= ORACLE_ROUNDING_CAP


def test_quaternions_reach_every_branch():
    q = ic.quaternions()
    assert q.shape == (4, ic.N_QUATERNIONS)
    sp, cr = ic.sinp(q), ic.cosr_cosp(q)
    fam = sp[:4]
    assert fam[0] == 1.0000000000000002 and fam[1] == -1.0000000000000002      # both clamp signs
    assert fam[2] == 1.0 and fam[3] == 0.9999999999999998                      # exactly 1, one ulp below
    assert (sp == -1.0).sum() + (sp == 1.0).sum() >= 1 and (sp > 1).any() and (sp < -1).any()
    assert -1e-15 < cr[0] < 0 and -1e-15 < cr[1] < 0                           # roll = atan2(0, -2.2e-16) = pi
    ref = ic.euler_reference()
    # the family's products with zero are exact, so a contracted kernel gives the same sinp and
    # cosr_cosp there; the witnesses are what a lost pragma moves: the reference's order clamps
    # (pitch = pi/2), either fused form takes the asin branch, 1.5e-8 rad lower
    x, y, z, w = q[:, 0]
    assert ic.sinp_contracted(x, y, z, w) == (fam[0], fam[0]) and 1 - 2 * ic.fma(x, x, y * y) == cr[0]
    wit = q[:, ic.WITNESS_AT]
    assert wit.shape[1] == ic.N_WITNESSES == len(ic.contraction_witnesses()) and np.abs(wit).min() > 0.05
    for j, col in enumerate(wit.T):
        assert sp[ic.WITNESS_AT][j] >= 1 and ref[1, ic.WITNESS_AT][j] == np.pi / 2
        for fused in ic.sinp_contracted(*col):
            assert fused < 1 and np.pi / 2 - np.arcsin(fused) > 1e-8
    assert ref[0, 0] == np.pi and ref[2, 0] == np.pi and ref[0, 1] == np.pi and ref[2, 1] == np.pi
    assert ref[1, 0] == np.pi / 2 and ref[1, 1] == -np.pi / 2 and ref[1, 2] == np.pi / 2
    assert 0 < np.pi / 2 - ref[1, 3] < 1e-7                                    # the asin branch
    norms = np.linalg.norm(q[:, ic.N_SPECIAL:], axis=0)
    for want in (0.5, 1.0, 2.0):
        assert (np.abs(norms - want) < 1e-12).sum() >= 300
    assert (np.abs(sp[ic.N_SPECIAL:]) >= 1).sum() >= 20                                  # norm 2 reaches the clamp too
    assert (q[:, :ic.N_SPECIAL] == 0).all(axis=0).sum() == 1                             # the zero quaternion
    nan_at = np.isnan(q)
    assert [int(np.nonzero(nan_at[:, j])[0][0]) for j in np.nonzero(nan_at.any(axis=0))[0]] == [0, 1, 2, 3]
    assert np.isnan(ref[:, nan_at.any(axis=0)]).any(axis=0).all() and not np.isnan(ref[:, ~nan_at.any(axis=0)]).any()
    # every prefix the GPU test cuts (255 and up) holds all the special ones
    assert nan_at.any(axis=0).nonzero()[0].max() < ic.N_SPECIAL <= 255


@pytest.mark.parametrize('count', ic.M7_COUNTS)
def test_bias_mean_is_the_row_by_row_sum(count):
    """np.mean over axis 0 of the reference's stacked rows = rows added one after another, divided
    by the count, bit for bit: the bias kernel's sum (32 loads at a time, added in order) relies on it."""
    name = f'M7_f{count}'
    imu = ic.merge_case(name)['imu']
    cnt = min(count, imu.shape[1])
    ref = ic.merge_reference(name)
    assert ref['first_valid_index'] == count
    for cols, got in ((slice(5, 8), ref['gyro_bias']), (slice(8, 11), ref['accel_bias'])):
        stat = [np.array([float(v) for v in imu[cols, r]]) for r in range(cnt)]
        s = np.zeros(3)
        for row in stat:
            s = s + row
        np.testing.assert_array_equal(np.mean(stat, axis=0), s / cnt)
        np.testing.assert_array_equal(got, s / cnt)


def test_merge_cases_state_their_info_fields():
    for (name, alt), (fvi, origin, n_fix, n_imu) in ic.CLAIMS.items():
        ref = ic.merge_reference(name, alt)
        got = (ref['first_valid_index'], ref['origin_row'], ref['n_fixes'], ref['n_imu'])
        assert got == (fvi, origin, n_fix, n_imu), (name, alt, got)
        assert len(ref['t']) == n_fix + n_imu
    for name in ic.merge_names():
        c = ic.merge_case(name)
        for alt in ic.merge_flags(name):
            ref = ic.merge_reference(name, alt)
            kept = ic.kept_rows(c['gps'], alt)
            assert ref['n_fixes'] == len(kept) and ref['origin_row'] == (kept[0] if len(kept) else -1)
            assert ref['first_valid_index'] == np.nonzero(~np.isnan(c['gps'][1]))[0][0]
            # the merged order is NumPy's stable argsort of [kept fixes..., IMU rows...]
            keys = np.concatenate([c['gps'][0, kept], c['imu'][0]])
            order = np.argsort(keys, kind='stable')
            np.testing.assert_array_equal(ref['t'].view(np.uint64), keys[order].view(np.uint64))
            np.testing.assert_array_equal(ref['etype'] == ic.IMU, order >= len(kept))
            np.testing.assert_array_equal(ref['src'], np.where(order >= len(kept), order - len(kept), order))


def _ties(ref):
    """Counts of adjacent equal-time pairs by kind: (GPS/GPS, IMU/IMU, GPS/IMU), and the longest run."""
    t, et = ref['t'], ref['etype']
    same = t[1:] == t[:-1]
    gg = int((same & (et[1:] == ic.GPS) & (et[:-1] == ic.GPS)).sum())
    ii = int((same & (et[1:] == ic.IMU) & (et[:-1] == ic.IMU)).sum())
    gi = int((same & (et[1:] != et[:-1])).sum())
    run = longest = 1
    for s in same:
        run = run + 1 if s else 1
        longest = max(longest, run)
    return gg, ii, gi, longest


def test_merge_cases_have_their_ties_and_drops():
    m1 = ic.merge_reference('M1')
    assert m1['n_imu'] == 0 and (m1['etype'] == ic.GPS).all() and np.isnan(m1['gyro_bias']).all()
    m2, g2 = ic.merge_reference('M2'), ic.merge_case('M2')['gps']
    assert not np.isnan(g2[1, 0]) and np.isnan(g2[2, 0]) and m2['first_valid_index'] != m2['origin_row']
    m3 = ic.merge_reference('M3')
    assert (m3['etype'] == ic.IMU).all() and m3['utm_origin'].tolist() == [0.0, 0.0]
    assert not np.isnan(m3['gyro_bias']).any()
    g4 = ic.merge_case('M4')['gps']
    only_alt = np.isnan(g4[3]) & ~np.isnan(g4[1]) & ~np.isnan(g4[2])
    assert only_alt.sum() == 4 and only_alt[1] and only_alt[-1]
    a, b = ic.merge_reference('M4', True), ic.merge_reference('M4', False)
    assert b['n_fixes'] - a['n_fixes'] == 4 and a['origin_row'] != b['origin_row']
    assert np.isnan(b['payload'][b['etype'] == ic.GPS, 2]).sum() == 4
    assert not np.array_equal(a['utm_origin'], b['utm_origin'])
    m5 = ic.merge_reference('M5')
    gg, ii, gi, longest = _ties(m5)
    assert gg >= 2 and ii >= 3 and gi >= 3 and longest >= 4
    assert m5['etype'][0] == ic.GPS and m5['etype'][-1] == ic.GPS and (m5['etype'][1:3] == ic.IMU).all()
    t_imu = ic.merge_case('M5')['imu'][0]
    assert (np.diff(t_imu) < 0).any()                                          # locally out of order
    at3 = np.nonzero(m5['t'] == 3.0)[0]
    assert m5['etype'][at3].tolist() == [ic.GPS, ic.IMU]                       # fixes first on a tie
    at7 = np.nonzero(m5['t'] == 7.0)[0]
    assert m5['etype'][at7].tolist() == [ic.GPS, ic.IMU, ic.IMU]               # the three-way tie
    m6 = ic.merge_reference('M6')
    assert (m6['t'] < 0).sum() == 3
    z = np.nonzero(m6['t'] == 0)[0]
    assert m6['etype'][z].tolist() == [ic.GPS, ic.GPS, ic.IMU, ic.IMU]
    assert np.signbit(m6['t'][z]).tolist() == [True, False, False, True]       # input order survives the tie
    assert ic.M7_N_IMU < max(ic.M7_COUNTS) and {31, 32, 33} <= set(ic.M7_COUNTS)
    mb = ic.merge_reference('M7_bias')
    np.testing.assert_array_equal(mb['gyro_bias'], ic.merge_case('M7_bias')['bias'][0])
    assert not np.array_equal(mb['gyro_bias'], ic.merge_reference('M7_f33')['gyro_bias'])
    for ng in ic.M8_N_GPS:
        for ni in ic.M8_N_IMU:
            for last in ('kept', 'dropped'):
                name = f'M8_{ng}_{ni}_{last}'
                c, ref = ic.merge_case(name), ic.merge_reference(name)
                assert c['gps'].shape == (4, ng) and c['imu'].shape == (11, ni)
                kept = ic.kept_rows(c['gps'])
                assert (kept[-1] == ng - 1) == (last == 'kept') and ng - 2 in kept
                assert 20 <= ng - len(kept) <= 90                                # scattered drops
                for col in (1, 2, 3):
                    assert np.isnan(c['gps'][col]).any()
                gg, ii, gi, _ = _ties(ref)
                assert gg >= 1 and (ni < 300 or (ii >= 1 and gi >= 1))


def test_nonfinite_cases_keep_a_fix_and_name_the_lowest_row():
    for name, (sensor, at, value, rejected, row) in ic.NONFINITE.items():
        gps, imu = ic.nonfinite_case(name)
        kept = ic.kept_rows(gps)
        assert len(kept) >= 1 and not np.isfinite(value)
        if sensor == 'gps':
            assert rejected == bool(set(at) & set(kept.tolist()))
            assert row == (min(set(at) & set(kept.tolist())) if rejected else None)
        else:
            assert rejected and row == min(at)
    # a dropped fix's time is never parsed: the oracle gives what it gave for the finite case
    gps, imu = ic.nonfinite_case('dropped_fix_nan')
    a, b = ic.reference(gps, imu), ic.merge_reference('M5')
    for k in ('etype', 't', 'src', 'payload'):
        np.testing.assert_array_equal(a[k], b[k])


def test_rows_are_what_the_reference_reads():
    r = ic.rows(np.array([[0.1, -0.0], [np.nan, 1e-9]]))
    assert r == [['0.1', 'nan'], ['-0.0', '1e-09']]
    assert float(r[1][0]) == 0 and np.signbit(float(r[1][0]))
    p = ic.padded(np.ones((2, 3)), 7)
    assert p.shape == (2, 10) and np.isnan(p[:, 3:]).all() and (p[:, :3] == 1).all()
    assert ref_ingest.gps_to_modified_utm([['0.0', '40.0', 'nan', '1.0']]) == []
