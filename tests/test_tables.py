"""CPU: the generated VP8 constant tables (webp_amd/csrc/vp8_tables.h, oracle/
vp8_tables.h) are identical to each other and to the values the reference's
Go source declares (tools/gen_vp8_tables.py): by the digests recorded from it,
and, where the reference checkout is present, value for value."""
import json
import os
import sys

from conftest import ROOT


def test_product_and_oracle_tables_identical():
    a = open(os.path.join(ROOT, "webp_amd", "csrc", "vp8_tables.h")).read()
    b = open(os.path.join(ROOT, "oracle", "vp8_tables.h")).read()
    assert a == b and "vp8_coeffs_proba0[1056]" in a


def header_values(txt, cname):
    start = txt.index(f"{cname}[")
    body = txt[txt.index("{", start) + 1:txt.index("};", start)]
    return [int(x) for x in body.replace(",", " ").split()]


def test_tables_match_reference_source():
    """Every table of the header has the length and SHA-256 recorded from the
    reference's Go source (tests/golden/reference_tables.json, written by
    tools/gen_vp8_tables.py); where the reference checkout is present, the
    values are also compared with the Go source itself."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_vp8_tables as G
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_tables.json")))
    txt = open(os.path.join(ROOT, "webp_amd", "csrc", "vp8_tables.h")).read()
    names = [c for _, _, c, _ in G.TABLES + G.ENC_TABLES] + [c for _, c in G.CATS]
    assert len(names) == 23 and sorted(names + ["inv_alpha"]) == sorted(pins)  # every pin is checked (inv_alpha:
    # tests/test_oracle.py)
    for cname in names:
        assert G.digest(header_values(txt, cname)) == pins[cname], cname
    if not os.path.isdir(G.REF):
        return
    srcs = {f: G.strip_comments(open(os.path.join(G.REF, f)).read()) for f in ("constants.go", "proba.go")}
    syms = G.symbols(srcs["constants.go"])
    tabs = [(c, t, G.values(srcs[f], g, syms)) for f, g, c, t in G.TABLES]
    for f, g, c, t in G.ENC_TABLES:
        src = G.strip_comments(open(os.path.join(os.path.dirname(G.REF), f)).read())
        tabs.append((c, t, G.values(src, g, syms)))
    for g, c in G.CATS:
        tabs.append((c, "uint8_t", G.cat_values(srcs["constants.go"], g)))
    for cname, ctype, vals in tabs:
        assert header_values(txt, cname) == vals, cname
