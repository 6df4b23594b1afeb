"""GPU: the G.711 transmission-codec augmentation (``air_g711_ragged`` through ``augment.g711_codec``), stage by stage
against tests/codec_oracle.py (audioop for the coding, float64 for the filters), its ragged layout, graph capture, and
``AugmentChain`` in front of the train step.

Tolerances.  The coding is integer arithmetic: bit for bit.  The decimator accumulates in fp32, so a 16-bit value can
round the other way where the exact pre-rounding value lies close to a half-integer: such samples are "contested" (within
0.02 LSB of x.5 - the fp32 bound ntaps * 2^-24 * sum|h| * max|x| * 32768 = 63 * 6e-8 * 1.855 * 0.48 * 32768 = 0.11 LSB is
never approached, a host fp32 FIR measures 0.0027 LSB), every other code must be equal.  At a contested sample the 16-bit
values differ by 1, so the codes are equal or neighbours, and neighbouring decoded levels lie one quantiser step apart -
the step of the coarser of the two segments when the pair straddles a segment boundary.  The interpolator is held to
2e-6 of the row's output scale, the bound tests/test_augment.py uses for a short response."""
import functools

import numpy as np
import pytest
import torch

import codec_oracle as co
from oracle.filler import fill_module_, synth_pcm

pytestmark = pytest.mark.gpu

TILE = 2048  # outputs per workgroup (GC_T, csrc/augment.hip)
LCAP = 9300
LENGTHS = [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 9297, 9298, LCAP]
LAW = [0, 1, 1, 0, -1, 1, 0, -1, 1, 0]  # -1: pass-through rows (a short and a long one)


def _dev(a, dtype=torch.int32):
    return torch.as_tensor(a, dtype=dtype).cuda()


def _pcm(lengths, cap, dtype=torch.float32, tail="zero", seed=9):
    """(B, cap) on the GPU; beyond its length a row is zero, or the worst value of its type."""
    x = synth_pcm(len(lengths), cap, seed=seed)
    if dtype == torch.int16:
        x = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    fill = 0 if tail == "zero" else (float("nan") if dtype == torch.float32 else 32767)
    for b, n in enumerate(lengths):
        x[b, n:] = fill
    return x.cuda()


# ------------------------------------------------------------------------------------------------------------ coding
@functools.lru_cache(maxsize=None)
def _all_values():
    from asvspoof2021_air_amd.augment import g711_codec
    k = torch.arange(-32768, 32768, dtype=torch.int32)
    x16 = k.to(torch.int16).reshape(1, -1).repeat(2, 1).cuda()
    xf = (k.float() / 32768.0).reshape(1, -1).repeat(2, 1).cuda()
    law = _dev([0, 1])
    out = {}
    for name, x in (("i16", x16), ("f32", xf)):
        y, codes = g711_codec(x, law, resample=False, normalize=False, return_codes=True)
        out[name] = (y.cpu(), codes.cpu())
    return out


@pytest.mark.parametrize("name", ["i16", "f32"])
def test_coding_equals_audioop_on_all_65536_values(name):
    y, codes = _all_values()[name]
    assert codes.dtype == torch.uint8 and codes.shape == (2, 65536) and y.dtype == torch.float32
    for law in (0, 1):
        enc, dec = co.tables(law)
        assert np.array_equal(codes[law].numpy(), enc), (name, law, int((codes[law].numpy() != enc).sum()))
        d = y[law].double().numpy() * 32768.0
        assert np.array_equal(d, dec[enc].astype(np.float64)), (name, law)


# --------------------------------------------------------------------------------------------- tiny filters: definition
def test_one_tap_filter_codes_every_second_sample():
    from asvspoof2021_air_amd.augment import g711_codec
    L = 2 * TILE + 77
    x = _pcm([L, L], L, seed=11)
    y, codes = g711_codec(x, _dev([0, 1]), fir=torch.ones(1).cuda(), normalize=False, return_codes=True)
    xh, y, codes = x.cpu().numpy(), y.cpu().numpy(), codes.cpu().numpy()
    assert codes.shape == (2, (L + 1) // 2)
    for law in (0, 1):
        want = co.encode(co.quantise(xh[law, ::2]), law)
        assert np.array_equal(codes[law], want)
        assert np.array_equal(y[law, ::2].astype(np.float64), 2.0 * co.decode(want, law) / 32768.0)
        assert not y[law, 1::2].any()


def test_three_tap_filter_equals_the_literal_double_loop():
    """Taps of 1/4, 1/2, 1/4 on 16-bit samples: every product and sum is exact in fp32, so codes AND y equal the float64
    double loop of the definition bit for bit; with general taps, y against the double loop over the kernel's own codes."""
    from asvspoof2021_air_amd.augment import g711_codec
    L = TILE + 301  # two workgroups, odd
    x16 = _pcm([L, L], L, torch.int16, seed=12)
    xh = x16.cpu().numpy().astype(np.float64) / 32768.0
    fir = np.array([0.25, 0.5, 0.25])
    y, codes = g711_codec(x16, _dev([0, 1]), fir=torch.tensor(fir, dtype=torch.float32).cuda(), normalize=False,
                          return_codes=True)
    gen = np.array([0.21, 0.55, 0.24])
    yg, cg = g711_codec(x16, _dev([0, 1]), fir=torch.tensor(gen, dtype=torch.float32).cuda(), normalize=False,
                        return_codes=True)
    for law in (0, 1):
        cw, yw = co.codec_definition(xh[law], fir, law)
        assert np.array_equal(codes[law].cpu().numpy(), cw)
        assert np.array_equal(y[law].double().cpu().numpy(), yw)
        # general taps: interpolate the kernel's own codes by the double loop
        v = co.decode(cg[law].cpu().numpy(), law) / 32768.0
        g32 = gen.astype(np.float32).astype(np.float64)
        want = np.array([2.0 * sum(g32[k] * v[(n + 1 - k) // 2] for k in range(3)
                                   if (n + 1 - k) % 2 == 0 and 0 <= (n + 1 - k) // 2 < len(v)) for n in range(L)])
        assert np.abs(yg[law].double().cpu().numpy() - want).max() <= 2e-6 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------------- ragged layout
@functools.lru_cache(maxsize=None)
def _ragged(dtype_name, normalize):
    from asvspoof2021_air_amd.augment import g711_codec
    dtype = torch.float32 if dtype_name == "f32" else torch.int16
    x = _pcm(LENGTHS, LCAP, dtype, tail="worst")
    keep = x.clone()
    law, ld = _dev(LAW), _dev(LENGTHS)
    y, codes = g711_codec(x, law, lengths=ld, normalize=normalize, return_codes=True)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(x.view(bits), keep.view(bits))  # the input is left as it was
    assert y.dtype == torch.float32 and y.shape == (len(LENGTHS), LCAP) and codes.shape == (len(LENGTHS), (LCAP + 1) // 2)
    return dict(x=x, law=law, ld=ld, y=y.cpu(), codes=codes.cpu())


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("dtype_name", ["f32", "i16"])
def test_ragged_rows_equal_the_call_on_each_utterance_alone(dtype_name, normalize):
    """Tails hold NaN / 32767: they are never read.  Row b is bit for bit the (1, L_b) call of the same entry point."""
    from asvspoof2021_air_amd.augment import g711_codec
    c = _ragged(dtype_name, normalize)
    assert bool(torch.isfinite(c["y"]).all())
    for b, n in enumerate(LENGTHS):
        xb = c["x"][b:b + 1, :n].contiguous()
        ya, ca = g711_codec(xb, c["law"][b:b + 1], normalize=normalize, return_codes=True)
        m = (n + 1) // 2
        assert torch.equal(c["y"][b, :n], ya[0].cpu()), (b, n, float((c["y"][b, :n] - ya[0].cpu()).abs().max()))
        assert torch.equal(c["codes"][b, :m], ca[0].cpu()), (b, n)
        assert int(torch.count_nonzero(c["y"][b, n:])) == 0 and int(torch.count_nonzero(c["codes"][b, m:])) == 0
        if LAW[b] < 0:
            xf = xb.float() / 32768.0 if dtype_name == "i16" else xb
            assert torch.equal(c["y"][b, :n], xf[0].cpu()) and int(torch.count_nonzero(c["codes"][b])) == 0
        else:
            assert int(torch.count_nonzero(c["codes"][b, :m])) > 0
    if dtype_name == "i16":  # the same bits as the fp32 call on the converted samples
        xf = (c["x"].float() / 32768.0)
        y2 = g711_codec(xf, c["law"], lengths=c["ld"], normalize=normalize)
        assert torch.equal(y2.cpu(), c["y"])


def test_host_lengths_and_out_are_honoured():
    from asvspoof2021_air_amd.augment import g711_codec
    c = _ragged("f32", True)
    out = torch.full((len(LENGTHS), LCAP), 7.0, device="cuda")
    with pytest.raises(ValueError):
        g711_codec(c["x"], c["law"], lengths=[0] + LENGTHS[1:], out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert g711_codec(c["x"], c["law"], lengths=LENGTHS, out=out) is out and torch.equal(out.cpu(), c["y"])


# -------------------------------------------------------------------------------------------- 63 taps against the oracle
SHAPE = (4, LCAP)
ROW_LAW = [0, 1, 0, 1]
ROW_LEN = [LCAP, 9297, TILE + 1, 5000]


@functools.lru_cache(maxsize=None)
def _oracle_case():
    from asvspoof2021_air_amd.augment import codec_lowpass, g711_codec
    x = synth_pcm(*SHAPE, seed=9)
    fir = codec_lowpass()
    xd, law, ld = x.cuda(), _dev(ROW_LAW), _dev(ROW_LEN)
    y, codes = g711_codec(xd, law, lengths=ld, normalize=False, return_codes=True)
    yn = g711_codec(xd, law, lengths=ld, normalize=True)
    f64 = fir.double().numpy()
    rows = [co.codec_row(x[b, :n].double().numpy(), f64, ROW_LAW[b], normalize=False) for b, n in enumerate(ROW_LEN)]
    return dict(x=x.numpy(), fir=f64, y=y.cpu().numpy(), yn=yn.cpu().numpy(), codes=codes.cpu().numpy(), rows=rows)


def test_codes_equal_the_oracle_except_at_contested_samples():
    c = _oracle_case()
    total = contested_total = flips = 0
    for b, n in enumerate(ROW_LEN):
        row, m = c["rows"][b], (n + 1) // 2
        got, want = c["codes"][b, :m], row["codes"]
        frac = row["u"] - np.floor(row["u"])
        contested = np.abs(frac - 0.5) <= 0.02
        total, contested_total = total + m, contested_total + int(contested.sum())
        diff = got != want
        flips += int(diff.sum())
        print("row %d: %d samples, %d contested, %d codes differ" % (b, m, int(contested.sum()), int(diff.sum())))
        assert not (diff & ~contested).any(), (b, int((diff & ~contested).sum()))
        law = ROW_LAW[b]
        step = np.maximum(co.step_at(got, law), co.step_at(want, law))
        gap = np.abs(co.decode(got, law).astype(np.int64) - co.decode(want, law).astype(np.int64))
        assert np.all(gap[contested] <= step[contested]), (b, int(gap.max()))
    print("contested %d of %d (%.2f %%), %d codes differ" % (contested_total, total, 100.0 * contested_total / total, flips))
    assert contested_total <= 0.05 * total  # on the oracle alone: expected share 2 * 0.02


def test_interpolation_of_the_kernels_own_codes():
    c = _oracle_case()
    for b, n in enumerate(ROW_LEN):
        m = (n + 1) // 2
        v = co.decode(c["codes"][b, :m], ROW_LAW[b]).astype(np.float64) / 32768.0
        want = co.interpolate(v, c["fir"], n)
        got = c["y"][b].astype(np.float64)
        scale, err = np.abs(want).max(), np.abs(got[:n] - want).max()
        print("row %d L %d: max |err| %.3g, scale %.3g" % (b, n, err, scale))
        assert err <= 2e-6 * scale, (b, err, scale)
        assert not got[n:].any() and not c["codes"][b, m:].any()
        # normalize: the row's own input peak, to one ulp; the same signal up to the gain
        px = np.abs(c["x"][b, :n]).max()
        pn = np.abs(c["yn"][b, :n]).max()
        assert abs(float(pn) - float(px)) <= float(np.spacing(np.float32(px))), (b, pn, px)
        assert not c["yn"][b, n:].any()
        gain = float(px) / scale
        assert np.abs(c["yn"][b, :n].astype(np.float64) - want * gain).max() <= 4e-6 * float(px)


# ---------------------------------------------------------------------------------------------------------- graph capture
def test_graph_replay_with_changed_lengths_and_laws_equals_the_eager_call():
    from asvspoof2021_air_amd.augment import g711_codec
    x = _pcm([LCAP] * 4, LCAP, seed=21)
    sets = [([LCAP, 100, TILE + 1, 5001], [0, 1, -1, 1]), ([1, LCAP, 9297, 2 * TILE], [1, -1, 0, 0]),
            ([TILE, TILE - 1, 3, LCAP], [-1, 0, 1, 1])]
    eager = [g711_codec(x, _dev(lw), lengths=_dev(ln)).cpu() for ln, lw in sets]
    ld, law, out = _dev(sets[0][0]), _dev(sets[0][1]), torch.empty(4, LCAP, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the stream's workspace and the default filter exist before the capture
        g711_codec(x, law, lengths=ld, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g711_codec(x, law, lengths=ld, out=out)
    for (ln, lw), want in list(zip(sets, eager))[::-1]:
        ld.copy_(_dev(ln))
        law.copy_(_dev(lw))
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), (ln, lw)


# ------------------------------------------------------------------------------------------------------ chain and trainer
B, CAP = 4, 9300
LENS = [[9300, 159, 6000, 4481], [4480, 9300, 2049, 9299], [2500, 9300, 8000, 300]]
STARTS = [[3, 0, 1, 0], [0, 2, 0, 1], [0, 5, 2, 0]]


def _chain(seed=1):
    from asvspoof2021_air_amd.augment import AugmentChain, ChannelAugment, CodecAugment, synthetic_ir_bank
    irs = synthetic_ir_bank(n_device=4, n_space=1, taps=128, seed=5)
    return AugmentChain(CodecAugment(p=0.7, seed=seed), ChannelAugment(irs=irs, p=0.7, seed=seed + 1)), irs


def test_chain_equals_the_two_calls_by_hand():
    from asvspoof2021_air_amd.augment import g711_codec, ir_convolve
    chain, irs = _chain()
    x, ld = _pcm(LENS[0], CAP, torch.int16, tail="worst", seed=31), _dev(LENS[0])
    labels = chain.prepare(B)
    drawn = [d.copy() for d in chain._prepared]
    assert labels.shape == (B, 2) and labels.dtype == torch.int64
    assert labels[:, 0].tolist() == [int(i) + 1 if i >= 0 else 0 for i in drawn[0]]
    assert labels[:, 1].tolist() == [int(i) + 1 if i >= 0 else 0 for i in drawn[1]]
    got = chain(x, lengths=ld)
    hand = g711_codec(x, _dev(drawn[0]), lengths=ld)
    hand = ir_convolve(hand, irs.cuda(), _dev(drawn[1]), True, lengths=ld)
    assert torch.equal(got, hand) and bool(torch.isfinite(got).all())
    assert chain._prepared is None
    # without a prepared draw the chain draws for itself, from the same generators
    other, _ = _chain()
    other.prepare(B)
    other(x, lengths=ld)
    want = [s.draw(B) for s in other.stages]
    seen = []
    for s in chain.stages:
        draw = s.draw
        s.draw = lambda n, draw=draw: seen.append(draw(n)) or seen[-1]
    chain(x, lengths=ld)
    assert all(np.array_equal(a, b) for a, b in zip(seen, want))


def _trainer(graph, augment=None, feat_len=48, seed=4242):
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    from asvspoof2021_air_amd.train import Trainer
    m = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(m)
    m = m.cuda()
    m._noise_seed = seed
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    tr = Trainer(m, loss_module=lossm, feat_len=feat_len, augment=augment)
    if graph:
        tr.enable_graph(segments=False)
    else:
        m.overlap_wgrad = False  # the capture is one chain; same launches eagerly
    return m, tr


def _batches():
    out = []
    for i in range(3):
        pcm = _pcm(LENS[i], CAP, torch.int16 if i == 1 else torch.float32, seed=500 + i)
        out.append((pcm, ((torch.arange(B) + i) % 3 != 0).long().cuda(), _dev(STARTS[i]), _dev(LENS[i])))
    return out


def test_ragged_step_with_the_chain_equals_the_hand_augmented_step_and_replays():
    batches = _batches()
    ends = []
    for mode in ("hand", "graph"):
        chain, _ = _chain(seed=7)
        m, tr = _trainer(mode == "graph", None if mode == "hand" else chain)
        losses, capture = [], None
        for i in range(5):  # two eager warm-up steps, the capture on batch 2, then batches 0 and 1 on replay
            pcm, lab, st, ln = batches[i % 3]
            if mode == "hand":
                pcm = chain(pcm, lengths=ln)
                assert pcm.dtype == torch.float32 and int(torch.count_nonzero(pcm[1, ln[1]:])) == 0
            losses.append(tr.step(pcm, lab, start=st, lengths=ln)[0].item())
            if mode == "graph" and i == 2:
                capture = tr._graph
                assert capture is not None and "ragged" in capture["key"]
        torch.cuda.synchronize()
        if mode == "graph":
            assert tr._graph is capture and len(capture["graphs"]) == 1  # one capture served the replays
        ends.append((losses, m.arena().flat.clone(), tr.loss.center.detach().clone(),
                     [s.rng.bit_generator.state for s in chain.stages]))
    (l0, w0, c0, r0), (l1, w1, c1, r1) = ends
    assert all(np.isfinite(l0)) and l0 == l1
    assert torch.equal(w0, w1) and torch.equal(c0, c1) and r0 == r1


def test_adversarial_step_takes_the_chains_labels():
    from asvspoof2021_air_amd.adversarial import AdversarialTrainer
    from asvspoof2021_air_amd.loss import AngularIsoLoss
    from asvspoof2021_air_amd.resnet import ResNet
    chain, irs = _chain(seed=3)
    pcm, lab, st, ln = _batches()[0]
    am = ResNet(3, 256, resnet_type="18", nclasses=2)
    fill_module_(am)
    am.set_attention_noise(None)
    lossm = AngularIsoLoss(256, r_real=0.9, r_fake=0.2, alpha=20.0)
    fill_module_(lossm)
    atr = AdversarialTrainer(am, (3, irs.shape[0] + 1), loss_module=lossm, feat_len=48, augment=chain)
    channels = chain.prepare(B)
    assert channels.shape == (B, 2) and int(channels[:, 0].max()) <= 2 and int(channels[:, 1].max()) <= irs.shape[0]
    loss, _ = atr.step(pcm, lab, channels=channels, start=st, lengths=ln)
    assert bool(torch.isfinite(loss).all()) and chain._prepared is None
