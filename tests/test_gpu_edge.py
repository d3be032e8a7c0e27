"""The device on the edge inputs (synth.edge_iq / edge_audio): silence from the first sample, signal
/ silence / signal with the recursive stages sitting in the denormals for tens of thousands of
samples, full-scale impulses and square waves, +-3 LSB noise, and loud input with all 32 bits in
use (the codec frames wrap with the AGC off).  Everything is compared exactly with the reference
firmware's recorded output (tests/golden/rxedge_*.npz, txedge_*.npz: a crc32 per 32-frame call and
three stored windows), or with the CPU oracle where the input is derived from those rows
(test_edge_oracle.py pins the oracle to the reference on them).

Lane c runs row kind c % 6, so every wave holds a silent lane, a denormal lane and a full-scale lane
side by side.  Lanes with the same input must agree bit for bit (checked on the device), and one lane
of each input is checked against the fixture on the host.  A failure names the lane and the first
32-frame call that differs, with the oracle's samples of that call."""
import numpy as np
import pytest

import edge_util as E
import oracle
import uhsdr_amd as U
from uhsdr_amd import synth

pytestmark = pytest.mark.gpu

NK = len(synth.EDGE_KINDS)
BURST = synth.EDGE_KINDS.index("burst")


def run_rx(cfg, rows, lane_row, N, nframes=None, stereo=False, mode=0, cw=False, keep=None):
    """rows [R][n][2] on lanes lane_row [C], calls of N frames enqueued back to back (per-call
    outputs, one synchronisation at the end; with cw, or keep(k) choosing the calls whose audio is
    kept, a synchronisation after the call).  Returns {"a1", "a0", "dst"}: device tensors [C][n(, 2)],
    {"sig", "en"} numpy with cw, "timeouts", and with keep {"a1": {call: numpy [C][N]}}."""
    import torch
    n = rows.shape[1] if nframes is None else nframes
    C, calls = len(lane_row), n // N
    chain = U.RxChain(cfg, channels=C, frames=N)
    if mode:
        chain.set_pipelined(mode)
    d_rows = torch.from_numpy(np.array(rows[:, :n])).cuda()
    d_lane = torch.from_numpy(np.asarray(lane_row, np.int64)).cuda()
    out = {}
    if keep is not None:
        lanes = d_rows.index_select(0, d_lane)
        audio = torch.empty((C, N), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        out["a1"] = {}
        for k in range(calls):
            chain.process(lanes[:, k * N:(k + 1) * N].contiguous(), audio, None)
            if keep(k):
                chain.synchronize()
                out["a1"][k] = audio.cpu().numpy()
        chain.synchronize()
        out["timeouts"] = chain.handoff_timeouts()
        chain.close()
        return out
    xs = [d_rows[:, k * N:(k + 1) * N].index_select(0, d_lane) for k in range(calls)]
    a1 = torch.empty((calls, C, N), dtype=torch.float32, device="cuda")
    a0 = torch.empty((calls, C, N), dtype=torch.float32, device="cuda") if stereo else None
    dst = torch.empty((calls, C, N, 2), dtype=torch.int32, device="cuda")
    if cw:
        sig = torch.zeros((C, N // 32), dtype=torch.uint8, device="cuda")
        en = torch.zeros((C, max(chain.cw_blocks_max, 1)), dtype=torch.float32, device="cuda")
        chain.set_cw_outputs(sig, en)
        sigs, ens = [], []
    torch.cuda.synchronize()
    for k in range(calls):
        if stereo:
            chain.process_stereo(xs[k], a1[k], a0[k], dst[k])
        else:
            chain.process(xs[k], a1[k], dst[k])
        if cw:
            chain.synchronize()
            sigs.append(sig.cpu().numpy())
            ens.append(en[:, :chain.cw_blocks_last].cpu().numpy())
    chain.synchronize()
    out["timeouts"] = chain.handoff_timeouts()
    chain.close()
    del xs
    out["a1"] = a1.permute(1, 0, 2).reshape(C, n)
    out["a0"] = a0.permute(1, 0, 2).reshape(C, n) if stereo else None
    out["dst"] = dst.permute(1, 0, 2, 3).reshape(C, n, 2)
    if cw:
        out["sig"], out["en"] = np.concatenate(sigs, axis=1), np.concatenate(ens, axis=1)
    return out


def representatives(lane_row):
    """first lane of every row, and for every lane the first lane with its input"""
    lane_row = np.asarray(lane_row)
    first = {int(r): int(np.flatnonzero(lane_row == r)[0]) for r in np.unique(lane_row)}
    return first, np.array([first[int(r)] for r in lane_row], np.int64)


def assert_lanes_agree(g, out, lane_row, keys, row_of=None):
    """lanes with the same input hold the same bits (on the device)"""
    import torch
    first, rep = representatives(lane_row)
    d_rep = torch.from_numpy(rep).cuda()
    for key in keys:
        t = out[key].view(torch.int32)
        ne = t != t.index_select(0, d_rep)
        if ne.any():
            per_frame = ne.reshape(ne.shape[0], ne.shape[1], -1).any(dim=2)
            frame = int(per_frame.any(dim=0).int().argmax())
            lane = int(per_frame[:, frame].int().argmax())
            r = int(lane_row[lane]) if row_of is None else row_of(int(lane_row[lane]))
            got = {key: out[key][lane].cpu().numpy()}
            raise AssertionError("lane differs from lane %d with the same input\n" % rep[lane]
                                 + E.describe(g, r, lane, (frame // 32, key, f"{int(per_frame.sum())} frames differ"), got))


def assert_rows_match_fixture(g, out, lane_row, keys, frame0=0):
    first, _ = representatives(lane_row)
    for r, lane in sorted(first.items()):
        got = {k: out[k][lane].cpu().numpy() for k in keys}
        bad = E.mismatch(g, r, got, frame0)
        if bad is not None:
            raise AssertionError(E.describe(g, r, lane, bad, got, frame0))


def keys_of(g):
    return ("a1", "a0", "dst") if g["stereo"] else ("a1", "dst")


@pytest.mark.parametrize("name", E.RX_NAMES)
def test_rx_edge_rows_match_reference(cuda, back, name):
    """130 channels (two full waves and a partial one), 102 calls of 2048 frames"""
    g = E.load_rx(name)
    lane_row = np.arange(130) % NK
    out = run_rx(E.rx_config(g), g["rows"], lane_row, 2048, stereo=g["stereo"])
    assert_lanes_agree(g, out, lane_row, keys_of(g))
    assert_rows_match_fixture(g, out, lane_row, keys_of(g))


def staggered_rows(g):
    """the six rows plus the burst row with its silence starting 32 .. 224 frames later; lane c:
    kind c % 6, the burst's silence 32 * ((c // 6) % 8) frames later.  -> (rows, lane_row)"""
    late = [synth.edge_iq("burst", [0], 0, g["frames"], base=g["base"], shift=32 * s, **g["base_kw"])[0] for s in range(1, 8)]
    rows = np.concatenate([g["rows"], np.stack(late)])
    c = np.arange(130)
    s = (c // NK) % 8
    lane_row = np.where((c % NK == BURST) & (s > 0), NK + s - 1, c % NK)
    return rows, lane_row


@pytest.mark.parametrize("name", ["p48_usb", "p55_usb", "p1_fm_sql0"])
def test_rx_staggered_silence_matches_oracle(cuda, back, name):
    """Lanes of one wave cross into the denormals in different 32-frame calls: 256-frame calls (so
    the one-kernel schedule runs too), every distinct input against the oracle."""
    g = E.load_rx(name)
    rows, lane_row = staggered_rows(g)
    assert len(np.unique(lane_row)) == NK + 7
    cfg = E.rx_config(g)
    ref_a1, _, ref_dst = oracle.OracleRx(U.build_plan(cfg), len(rows)).process2(rows, threads=8)
    out = run_rx(cfg, rows, lane_row, 256)
    base_row = lambda r: r if r < NK else BURST  # noqa: E731
    assert_lanes_agree(g, out, lane_row, ("a1", "dst"), row_of=base_row)
    first, _ = representatives(lane_row)
    for r, lane in sorted(first.items()):
        for key, ref in (("a1", ref_a1), ("dst", ref_dst)):
            got = out[key][lane].cpu().numpy()
            ne = (got.view(np.uint32) != ref[r].view(np.uint32)).reshape(len(got), -1).any(axis=1)
            if ne.any():
                f = int(np.argmax(ne))
                raise AssertionError(f"rxedge_{name} row {r} (burst shifted by {32 * max(r - NK + 1, 0)}) lane {lane}: "
                                     f"{int(ne.sum())} frames of {key} differ, first in call {f // 32}\n"
                                     f"  device: {got[f // 32 * 32:f // 32 * 32 + 32].ravel()[:16]!r}\n"
                                     f"  oracle: {ref[r][f // 32 * 32:f // 32 * 32 + 32].ravel()[:16]!r}")
        if base_row(r) == BURST:
            assert E.denormals(ref_a1[r]) >= 20000, f"row {r}: the shifted silence no longer reaches the denormals"


@pytest.mark.parametrize("name", E.RX_NAMES)
def test_rx_256_frame_calls(cuda, back, name):
    """65 channels, 816 calls of 256 frames: the call size at which the one-kernel schedule runs
    (a 2048-frame call has two front launches, so there the handle keeps its own choice)"""
    g = E.load_rx(name)
    lane_row = np.arange(65) % NK
    out = run_rx(E.rx_config(g), g["rows"], lane_row, 256, stereo=g["stereo"])
    assert_lanes_agree(g, out, lane_row, keys_of(g))
    assert_rows_match_fixture(g, out, lane_row, keys_of(g))


def test_rx_isr_sized_calls(cuda):
    """32-frame calls over the first 110,592 frames (past the first denormal sample); the audio of
    every 256th call and of the last one"""
    g = E.load_rx("p48_usb")
    n = 110592
    assert g["win_start"][BURST][1] + 2048 < n
    lane_row = np.arange(65) % NK
    last = n // 32 - 1
    out = run_rx(E.rx_config(g), g["rows"], lane_row, 32, nframes=n, keep=lambda k: k % 256 == 255 or k == last)
    assert len(out["a1"]) == n // 32 // 256 + 1
    _, rep = representatives(lane_row)
    for k, a in out["a1"].items():
        assert np.array_equal(a.view(np.uint32), a.view(np.uint32)[rep]), f"call {k}: lanes with the same input differ"
        for r in range(NK):
            bad = E.mismatch(g, r, {"a1": a[r]}, frame0=32 * k)
            if bad is not None:
                raise AssertionError(E.describe(g, r, r, bad, {"a1": a[r]}, 32 * k))


@pytest.mark.parametrize("mode", [2, 3], ids=["device_handoff", "persistent"])
@pytest.mark.parametrize("name", ["p48_usb", "p48_agcoff"])
def test_rx_pipelined_modes(cuda, name, mode):
    """256-frame calls enqueued back to back: the serial result, the fixture, and no poll giving up"""
    import torch
    g = E.load_rx(name)
    lane_row = np.arange(65) % NK
    serial = run_rx(E.rx_config(g), g["rows"], lane_row, 256)
    out = run_rx(E.rx_config(g), g["rows"], lane_row, 256, mode=mode)
    assert out["timeouts"] == 0
    assert_lanes_agree(g, out, lane_row, ("a1", "dst"))
    assert_rows_match_fixture(g, out, lane_row, ("a1", "dst"))
    for key in ("a1", "dst"):
        assert torch.equal(out[key].view(torch.int32), serial[key].view(torch.int32)), f"{key}: not the serial result"


def test_rx_cw_side_outputs(cuda, back):
    """Goertzel energies and ads.CW_signal on the p4_cw rows"""
    g = E.load_rx("p4_cw")
    lane_row = np.arange(65) % NK
    out = run_rx(E.rx_config(g), g["rows"], lane_row, 2048, cw=True)
    assert out["en"].shape[1] == g["cw_energy"].shape[1]
    for c, r in enumerate(lane_row):
        assert np.array_equal(out["sig"][c], g["cw_signal"][r]), f"CW signal state, lane {c} ({synth.EDGE_KINDS[r]})"
        ne = np.flatnonzero(out["en"][c].view(np.uint32) != g["cw_energy"][r].view(np.uint32))
        assert len(ne) == 0, (f"Goertzel energy, lane {c} ({synth.EDGE_KINDS[r]}): {len(ne)} blocks differ, first {ne[0]}: "
                              f"{out['en'][c][ne[0]]!r} vs {g['cw_energy'][r][ne[0]]!r}")
    assert_rows_match_fixture(g, out, lane_row, ("a1", "dst"))


TX_CASES = [(n, False) for n in E.TX_NAMES] + [("usb", True)]


@pytest.mark.parametrize("name,pipelined", TX_CASES, ids=[f"{n}{'_pipelined' if p else ''}" for n, p in TX_CASES])
def test_tx_edge_rows_match_reference(cuda, name, pipelined):
    """65 channels tiled over silence, audio / silence / audio and the full-scale square wave, 256-frame
    calls enqueued back to back"""
    import torch
    g = E.load_tx(name)
    C, N, n = 65, 256, g["frames"]
    lane_row = np.arange(C) % len(g["kinds"])
    chain = U.TxChain(E.tx_config(g), channels=C, frames=N)
    chain.set_pipelined(pipelined)
    d_rows = torch.from_numpy(np.array(g["rows"])).cuda()
    d_lane = torch.from_numpy(lane_row).cuda()
    xs = [d_rows[:, k * N:(k + 1) * N].index_select(0, d_lane) for k in range(n // N)]
    iq = torch.empty((n // N, C, N, 2), dtype=torch.int32, device="cuda")
    a0 = torch.empty((n // N, C, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k, x in enumerate(xs):
        chain.process(x, iq[k], a0[k])
    chain.join()
    torch.cuda.synchronize()
    chain.close()
    out = {"iq": iq.permute(1, 0, 2, 3).reshape(C, n, 2), "a0": a0.permute(1, 0, 2).reshape(C, n)}
    first, rep = representatives(lane_row)
    d_rep = torch.from_numpy(rep).cuda()
    for key, t in out.items():
        assert torch.equal(t.view(torch.int32), t.view(torch.int32).index_select(0, d_rep)), f"{key}: lanes with the same input differ"
    for r, lane in sorted(first.items()):
        got = {k: t[lane].cpu().numpy() for k, t in out.items()}
        bad = E.mismatch(g, r, got)
        if bad is not None:
            raise AssertionError(E.describe(g, r, lane, bad, got).replace("rxedge_", "txedge_"))
