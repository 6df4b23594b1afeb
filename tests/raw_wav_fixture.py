"""A small synthetic tree for the six ``.wav`` classes of raw_dataset.py, shared by tests/golden/make_golden_raw_wav.py
(which runs the REFERENCE's classes over it, the waveform read stubbed) and tests/test_wav_cpu.py (which runs this
package's classes over the same tree with real files).  ``write(path, k)`` creates file number k.

    vcc/spoof/<team>/<pair>/<utt>.wav            VCC2020Raw: tag = the directory two levels up
    vcc/bonafide/<set>/<speaker>/<utt>.wav       filename = the last three path components joined by '_'
    a2015/wav/<part>/<speaker>/<file>.wav        ASVspoof2015Raw, protocols a2015/CM_protocol/cm_{train.trn,develop.ndx,evaluation.ndx}
    aug1/<part>/<name>_<channel>.wav             ...withTransmission / ...withCompression
    aug2/<part>/<name>_<channel>_<device>.wav    ...AndDevice
    proto/ASVspoof2019.LA.cm.<part>.trl.txt      train / dev; eval: aug?/LA/ASVspoof2019_LA_cm_protocols/
"""
import os

VCC_SPOOF = ["T02/TEF1-SEF2/E30003", "T01/TEF1-SEF1/E30001", "T01/TEF1-SEF1/E30002", "T10/TMF1-SEM1/E30001"]
VCC_BONAFIDE = ["source/SEF1/E10002", "source/SEF1/E10001", "target_task1/TEF1/E20001"]
A2015 = {"train": [("T1", "T1_000001", "human", "human"), ("T1", "T1_000002", "S3", "spoof"), ("T2", "T2_000001", "S1", "spoof")],
         "dev": [("D3", "D3_100001", "S5", "spoof"), ("D3", "D3_100002", "human", "human")],
         "eval": [("E7", "E7_200001", "S10", "spoof"), ("E8", "E8_200002", "human", "human"), ("E8", "E8_200003", "S6", "spoof")]}
A2015_PROTOCOL = {"train": "cm_train.trn", "dev": "cm_develop.ndx", "eval": "cm_evaluation.ndx"}
AUG_PROTOCOL = {"train": [("LA_0079", "LA_T_1000001", "-", "bonafide"), ("LA_0080", "LA_T_1000002", "A03", "spoof"),
                          ("LA_0081", "LA_T_1000003", "A07", "spoof")],
                "dev": [("LA_0069", "LA_D_2000001", "A01", "spoof"), ("LA_0070", "LA_D_2000002", "-", "bonafide")],
                "eval": [("LA_0001", "LA_E_3000001", "A05", "spoof"), ("LA_0002", "LA_E_3000002", "-", "bonafide")]}
AUG1 = ["g711[law=u]", "amr[br=5k9]", "no-channel"]          # one file per (protocol file, channel) ...
AUG2 = [("g722[br=64k]", "OktavaML19"), ("silk[br=5k]", "iPhone7")]  # ... or per (file, channel, device)
CLASSES = ["VCC2020Raw", "ASVspoof2015Raw", "ASVspoof2019LARaw_withTransmission", "ASVspoof2019LARaw_withTransmissionAndDevice",
           "ASVspoof2019DFRaw_withCompression", "ASVspoof2019DFRaw_withCompressionAndDevice"]


def build(root, write):
    k = 0

    def put(*parts):
        nonlocal k
        path = os.path.join(root, *parts)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        write(path, k)
        k += 1

    for rel in VCC_SPOOF:
        put("vcc", "spoof", rel + ".wav")
    for rel in VCC_BONAFIDE:
        put("vcc", "bonafide", rel + ".wav")
    with open(os.path.join(root, "vcc", "spoof", "README.txt"), "w") as f:
        f.write("not audio\n")
    os.makedirs(os.path.join(root, "a2015", "CM_protocol"))
    for part, rows in A2015.items():
        for speaker, name, tag, label in rows:
            put("a2015", "wav", part, speaker, name + ".wav")
        with open(os.path.join(root, "a2015", "CM_protocol", A2015_PROTOCOL[part]), "w") as f:
            f.write("".join("%s %s %s %s\n" % r for r in rows))
    os.makedirs(os.path.join(root, "proto"))
    for part, rows in AUG_PROTOCOL.items():
        for i, (speaker, name, tag, label) in enumerate(rows):
            for ch in AUG1[i % 2:]:
                put("aug1", part, "%s_%s.wav" % (name, ch))
            for ch, dev in AUG2[:1 + i % 2]:
                put("aug2", part, "%s_%s_%s.wav" % (name, ch, dev))
        text = "".join("%s %s - %s %s\n" % r for r in rows)
        if part == "eval":
            for db in ("aug1", "aug2"):
                d = os.path.join(root, db, "LA", "ASVspoof2019_LA_cm_protocols")
                os.makedirs(d)
                with open(os.path.join(d, "ASVspoof2019.LA.cm.eval.trl.txt"), "w") as f:
                    f.write(text)
        else:
            with open(os.path.join(root, "proto", "ASVspoof2019.LA.cm.%s.trl.txt" % part), "w") as f:
                f.write(text)
    return k


def cases(mod, root):
    """name -> a constructor of ``mod``'s class over the tree (positional arguments in the reference's order)."""
    j = lambda *p: os.path.join(root, *p)
    out = {"VCC2020Raw": lambda: mod.VCC2020Raw(j("vcc", "spoof"), j("vcc", "bonafide"))}
    for part in ("train", "dev", "eval"):
        out["ASVspoof2015Raw/" + part] = lambda part=part: mod.ASVspoof2015Raw(j("a2015", "wav"), j("a2015", "CM_protocol"), part)
        for name in CLASSES[2:]:
            db = "aug2" if name.endswith("AndDevice") else "aug1"
            # eval reads its protocol from the database tree: path_to_protocol is then unused
            out["%s/%s" % (name, part)] = lambda name=name, db=db, part=part: getattr(mod, name)(
                j(db), j("proto") if part != "eval" else j("nowhere"), part)
    return out


def record(ds, root):
    """What the golden fixture pins of a dataset: its length, the order of its files (where it lists them), and every
    item's metadata (item[1:]).  ``files`` are relative to the tree."""
    rel = lambda p: os.path.relpath(p, root).replace(os.sep, "/")
    files = None
    if hasattr(ds, "all_files"):
        files = [rel(p) for p in ds.all_files]
    elif hasattr(ds, "all_bonafide"):
        files = [rel(p) for p in ds.all_bonafide] + [rel(p) for p in ds.all_spoof]
    return {"len": len(ds), "files": files, "meta": [[str(v) for v in ds[i][1:]] for i in range(len(ds))],
            "tag": dict(ds.tag) if hasattr(ds, "tag") else None, "label": dict(ds.label) if hasattr(ds, "label") else None}
