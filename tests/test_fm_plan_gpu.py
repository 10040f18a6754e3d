"""Every handle of tests/fm_plan_cases.py created on the device: sdrfm_kernel_name right after create and after one small device-pointer call (2 streams,
8 D Da 8 samples on 16-byte aligned rows) against tests/golden/fm_plan_mi355x.json, what the library answered on an MI355X before its create-time
decisions moved into csrc/sdrfm_fm_plan.h.  tests/test_fm_plan_cpu.py holds the whole plan to the same record without a device."""
import pytest

import fm_plan_cases as pc

pytestmark = pytest.mark.gpu
RECORD = pc.load_record()


@pytest.fixture(scope="module")
def rows(pkg):
    """device I/Q rows per call size, made once"""
    import torch
    made = {}

    def get(n):
        if n not in made:
            iq = torch.from_numpy(pkg.make_iq(pc.N_STREAMS, n, mode="fm", first_id=40)).cuda()
            assert iq.data_ptr() % 16 == 0 and iq.stride(0) % 16 == 0
            made[n] = iq
        return made[n]
    return get


@pytest.mark.parametrize("cid", [c[0] for c in pc.cases()])
def test_the_handle_names_the_recorded_kernels(pkg, rows, cid):
    import torch
    rec = RECORD[cid]
    T, D, Ta, Da, flags = rec["T"], rec["D"], rec["Ta"], rec["Da"], rec["flags"]
    h, g = pc.taps(pkg, T, D, Ta, Da, rec["taps"])
    n = pc.call_nsamp(D, Da)
    cfg = pkg.FmConfig(fir_coeffs=h, audio_coeffs=g, fir_decim=D, audio_decim=Da, n_streams=pc.N_STREAMS, max_bytes_per_call=2 * n,
                       force_generic=bool(flags & 1), bit_exact=bool(flags & 4), guard_worst_case=bool(flags & 8))
    with pkg.FmDemod(cfg) as dm:
        assert dm.kernel_name == rec["name_after_create"]
        assert (dm.q_guard() is not None) == bool(rec["plan"]["geo"]["has_q"])
        audio = torch.zeros((pc.N_STREAMS, dm.audio_count(2 * n) + 1), dtype=torch.float32, device="cuda")
        assert dm.process_batch_device(rows(n), audio) == rec["n_audio"]
        dm.synchronize()
        assert dm.kernel_name == rec["name_after_call"]
