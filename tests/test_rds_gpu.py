"""GPU checks of RDS reception where it matters: the default shape against the reference bit for bit on station input, and the whole
receiver — RdsDemod on device tensors, RdsSync per row, the block criterion of tests/test_rds_ref.py — at the machine-filling batch."""
import numpy as np
import pytest

from rds_ref import check_blocks, oracle_d, rds_ref, station_samples
from test_rds_shapes_gpu import _bits, _device_d

pytestmark = pytest.mark.gpu

FS, D, DR = 2.4e6, 10, 25


def _setup(pkg):
    return pkg.lowpass_taps(64, 120e3 / FS), pkg.stereo_pilot_taps(101, FS / D), pkg.rds_lowpass_taps(255, FS / D), pkg.rds_gain(D, FS)


def _demod(pkg, ns, nbytes, **kw):
    h, b, g, gain = _setup(pkg)
    return pkg.RdsDemod(pkg.RdsConfig(fir_coeffs=h, pilot_coeffs=b, rds_coeffs=g, pilot_min=0.05, rds_gain=gain, fir_decim=D, rds_decim=DR,
                                      n_streams=ns, max_bytes_per_call=nbytes, **kw))


def test_default_shape_is_the_reference_bit_for_bit_on_stations(pkg, oracle_mod):
    """Every stage behind d is a written fmaf, a product or a correctly rounded quotient, so the device's w should be the fp32-faithful
    reference's on the device's own d, bit for bit.  Were it not, the yardstick would be the reference's own rounding noise: the worst
    error relative to each stream's RMS |w| at most 4 x the fp32-against-exact64 figure of that stream (tests/test_rds_ref.py measures
    7.3e-6 and 8.1e-6 of RMS on such streams)."""
    h, b, g, gain = _setup(pkg)
    ns, nsamp = 4, 600000
    sent = pkg.rds_encode_groups(0xD3C2, "GRAFT FM", "RDS on the GPU..")
    iq = np.stack([pkg.make_iq_rds(1, nsamp, sent, rds_phase=0.7 * s, clock_ppm=(0, 100, -100, 0)[s], first_id=60 + s)[0] for s in range(ns)])
    ds = _device_d(pkg, oracle_mod, h, D, iq)
    with _demod(pkg, ns, 2 * nsamp) as rd:
        name = rd.kernel_name
        bb, pc = rd.process_batch(iq)
    assert name.startswith("rds-fast"), name
    for s in range(ns):
        r32 = rds_ref(ds[s], b, g, 0.05, gain, DR)
        r64 = rds_ref(ds[s], b, g, 0.05, gain, DR, exact64=True)
        rms = float(np.sqrt(np.mean(np.abs(r64["w"][50:]) ** 2)))
        own = float(np.abs(r32["w"].astype(np.complex128) - r64["w"]).max()) / rms
        dev = float(np.abs(bb[s].astype(np.complex128) - r64["w"]).max()) / rms
        same = np.array_equal(_bits(bb[s]), _bits(r32["w"]))
        print("stream %d: RMS |w| %.3g; reference fp32 against exact64 %.3g of RMS, device against exact64 %.3g of RMS; device == reference "
              "bitwise: %s; pilot count %d of %d" % (s, rms, own, dev, same, int(pc[s]), ds[s].size))
        assert int(pc[s]) == r32["count"]
        assert same, (s, float(np.abs(bb[s].astype(np.complex128) - r32["w"]).max()))


def test_receiver_end_to_end_at_the_machine_filling_batch(pkg):
    """256 rows x 13 calls of 480 000 bytes (1.3 s, 14 groups): 32 distinct stations (own PI, PS, carrier offset, rds_phase; a quarter
    of them with the crystal +-100 ppm off) repeated over the rows, with a pilot-less mono row after every three."""
    import torch
    ns, call_bytes, n_calls = 256, 480000, 13
    nsamp = call_bytes // 2 * n_calls
    n_groups = 14
    assert station_samples(n_groups) <= nsamp
    stations = []
    for k in range(32):
        sent = pkg.rds_encode_groups(0x1000 + 0x111 * k, "RADIO %02d" % k, "row %02d of the batch" % k, pty=k % 32)
        ppm = (100.0, -100.0)[(k // 4) % 2] if k % 4 == 0 else 0.0
        stations.append((sent, pkg.make_iq_rds(1, nsamp, sent, rds_phase=(np.pi / 2) * k / 7.0, clock_ppm=ppm, first_id=9000 + k)[0]))
    monos = [pkg.make_iq_rds(1, nsamp, stations[0][0], pilot=False, first_id=9500 + k)[0] for k in range(4)]
    rows = [("mono", monos[(r // 4) % 4]) if r % 4 == 3 else ("station", (r - r // 4) % 32) for r in range(ns)]
    assert len({k for kind, k in rows if kind == "station"}) == 32
    d_bb = torch.zeros((ns, 2 * 1000), dtype=torch.float32, device="cuda")
    d_pc = torch.zeros(ns, dtype=torch.int32, device="cuda")
    d_iq = torch.empty((ns, call_bytes), dtype=torch.uint8, device="cuda")
    host = np.empty((ns, call_bytes), np.uint8)
    syncs = [pkg.RdsSync(FS / D / DR) for _ in range(ns)]
    got = [[] for _ in range(ns)]
    with _demod(pkg, ns, call_bytes) as rd:
        assert rd.kernel_name.startswith("rds-fast"), rd.kernel_name
        for c in range(n_calls):
            for r, (kind, k) in enumerate(rows):
                host[r] = (k if kind == "mono" else stations[k][1])[c * call_bytes:(c + 1) * call_bytes]
            d_iq.copy_(torch.from_numpy(host))
            torch.cuda.synchronize()
            n = rd.process_batch_device(d_iq, d_bb, d_pc)
            rd.synchronize()
            assert rd.kernel_name.startswith("rds-fast"), rd.kernel_name
            assert n == call_bytes // 2 // D // DR
            bb = d_bb[:, :2 * n].cpu().numpy()
            pcs = d_pc.cpu().numpy()
            for r, (kind, k) in enumerate(rows):
                got[r] += syncs[r].push(bb[r])
                if kind == "mono":
                    assert c == 0 or pcs[r] == 0, (r, c, int(pcs[r]))
                elif c > 0:
                    assert pcs[r] == call_bytes // 2 // D, (r, c, int(pcs[r]))
    n_ok = 0
    for r, (kind, k) in enumerate(rows):
        if kind == "mono":
            assert got[r] == [] and syncs[r].stats()["groups"] == 0, r
            continue
        sent = stations[k][0]
        first, ok = check_blocks(sent, got[r], n_groups, "row %d (station %d)" % (r, k))
        n_ok += ok
        info = pkg.rds_parse(got[r])
        assert info["pi"] == sent[0][0] and info["ps"] == "RADIO %02d" % k, (r, info)
        assert info["text"] == "row %02d of the batch" % k, (r, info)
    for s in syncs:
        s.close()
    print("256 rows x %d calls: %d station rows of 32 stations decoded, %d blocks ok; 64 mono rows: no group, pilot_count 0" % (
        n_calls, sum(1 for kind, _ in rows if kind == "station"), n_ok))
