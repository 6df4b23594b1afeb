"""GPU: the records of the device chain (csrc/eval_metrics.hip) against the numpy model of its walk
(eval_walk_oracle.walk_model, pinned to the host functions by test_eval_groups_cpu.py), word for word.  Without groups
(n_groups = 0, ops.eval_det_min) and with them (ops.eval_det_min_grouped) the same kernels run, so the comparison of a
group's record with the pooled call on the compacted subset (test_eval_groups_gpu.py) is not the only record-level check.

What the model defines is compared, with ``==`` on the bytes:
  - of every record the four counts, n_distinct and reserved[0] (the ids out of range, in record 0);
  - of a record with both classes also has_dcf and the eer_* fields, and with weights the dcf_* fields.
The model leaves the other words zero where the header calls them meaningless: the indices and scores of a record that
lacks a class (n = 1, and groups of the small sizes), and the dcf_* fields without weights (has_dcf = 0)."""
import numpy as np
import pytest
import torch

from eval_walk_oracle import WALK_GROUPS, WALK_KINDS, WALK_SIZES, walk_case, walk_model, walk_weights
from test_eval_groups_gpu import COUNT_FIELDS, FIELDS

pytestmark = pytest.mark.gpu


def device_records(s, lab, grp, n_groups, negate, weights):
    from asvspoof2021_air_amd import eval_metrics as em, ops
    ds, dl = torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda()
    recs = torch.empty((n_groups + 1) * ops.EVAL_RECORD_WORDS, dtype=torch.int32, device="cuda")
    if n_groups == 0:
        ws = torch.empty(ops.eval_workspace_bytes(s.size), dtype=torch.uint8, device="cuda")
        c1, c2 = (None, None) if weights is None else weights[0]
        ops.eval_det_min(ds, dl, recs, ws, negate=negate, c1=c1, c2=c2)
    else:
        ws = torch.empty(ops.eval_workspace_bytes_grouped(s.size, n_groups), dtype=torch.uint8, device="cuda")
        c12 = None if weights is None else torch.tensor(weights, dtype=torch.float64).cuda()
        ops.eval_det_min_grouped(ds, dl, torch.from_numpy(grp).cuda(), n_groups, recs, ws, negate=negate, c12=c12)
    return recs.cpu().numpy().view(em._RECORD)


@pytest.mark.parametrize("n", WALK_SIZES)
def test_records_equal_the_walk_model(n):
    assert "reserved" not in FIELDS
    seen_out_of_range = False
    for n_groups in WALK_GROUPS:
        for j, kind in enumerate(WALK_KINDS):
            s, lab, grp = walk_case(n, n_groups, kind, 10 * n + j)
            for negate in (False, True):
                for weights in (None, walk_weights(n_groups)):
                    tag = (n, n_groups, kind, negate, weights is not None)
                    got = device_records(s, lab, grp, n_groups, negate, weights)
                    want = walk_model(s, lab, grp, n_groups, negate, weights)
                    assert got.shape == want.shape == (n_groups + 1,)
                    seen_out_of_range |= int(want[0]["reserved"][0]) > 0
                    for r in range(n_groups + 1):
                        fields = COUNT_FIELDS + ("n_distinct",)
                        if int(want[r]["n_tar"]) and int(want[r]["n_non"]):
                            fields = tuple(f for f in FIELDS if weights is not None or not f.startswith("dcf_"))
                        for f in fields:
                            assert got[r][f].tobytes() == want[r][f].tobytes(), (tag, r, f, got[r][f], want[r][f])
                        assert int(got[r]["reserved"][0]) == int(want[r]["reserved"][0]), (tag, r)
    assert seen_out_of_range == (n >= 4095)
