"""CPU tests that pin the build to data the reference itself holds.

* RX segmentation: the known answers of the reference's ldpc_segmenter_test (tests/unittests/phy/upper/channel_coding/
  ldpc/ldpc_segmenter_test_data.h:43-53: TBS, base graph, number of segments, segment length K*Z; the .dat payload
  files are not in the reference tree, these four numbers per case are). Checked for the product's host segmenter
  (srsran_projectvtlmo_amd.segmentation) and the oracle.
* Base-graph tables: csrc/ldpc_base_graphs.inc, which the HIP library and the oracle both compile, compared byte for
  byte (below its leading comment) with the shift coefficients of the reference's ldpc_luts_impl.cpp as stored in
  tests/golden/ldpc_base_graph_shifts.json (extracted by tests/golden/make_base_graph_shifts.py through
  tools/gen_ldpc_tables.py). HIP-vs-oracle parity cannot see a table error both share; this test can.
"""
from pathlib import Path

import pytest

import oracle as O
from srsran_projectvtlmo_amd import segmentation as S

ROOT = Path(__file__).resolve().parent.parent

# (tbs, bg, nof_segments, segment_length) -- ldpc_segmenter_test_data.h:43-53
SEGMENTER_KAT = [
    (96, 1, 1, 132), (600, 1, 1, 616), (4000, 1, 1, 4224), (12000, 1, 2, 6336), (40000, 1, 5, 8448),
    (96, 2, 1, 200), (320, 2, 1, 440), (600, 2, 1, 720), (4000, 2, 2, 2080), (12000, 2, 4, 3200),
    (40000, 2, 11, 3840),
]


@pytest.mark.parametrize("tbs,bg,nseg,seglen", SEGMENTER_KAT)
def test_segmenter_known_answers(tbs, bg, nseg, seglen):
    K = 22 if bg == 1 else 10
    # the channel allocation only sets E; any valid one works for C, Z and K*Z
    for seg in (S.segment_rx(tbs, bg, 5000, 2, 1), ):
        assert len(seg) == nseg
        assert all(K * m.lifting_size == seglen for m in seg)
    ref = O.segment_rx(tbs, bg, 5000, 2, 1)
    assert len(ref) == nseg and all(K * m["Z"] == seglen for m in ref)


def test_base_graph_tables_match_reference_luts():
    import json
    import re
    golden = json.loads((ROOT / "tests" / "golden" / "ldpc_base_graph_shifts.json").read_text())
    assert golden["columns"] == ["bg", "row", "col"] + [f"s{i}" for i in range(8)]
    want = [f"LDPC_EDGE({', '.join(str(x) for x in e)})" for e in golden["edges"]]
    assert sum(1 for e in golden["edges"] if e[0] == 1) == 316 and sum(1 for e in golden["edges"] if e[0] == 2) == 197
    committed = (ROOT / "srsran_projectvtlmo_amd" / "csrc" / "ldpc_base_graphs.inc").read_text()
    # every line of the table outside its leading comment, in order: the generator's output, byte for byte
    body = re.sub(r"\A/\*.*?\*/\n", "", committed, flags=re.S)
    assert body == "\n".join(want) + "\n"
