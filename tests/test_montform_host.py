"""The Montgomery output form (H2W_OPT_OUTPUT_FORM) without a GPU: the arithmetic of csrc/montform.h on the host, and the map of the cells
that the ranged pass converts."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def test_every_route_of_the_conversion_on_the_host(tmp_path):
    """tests/cpp/montform_check.cpp: every route (two, three, four, eight words, a run-time row count, by width) against 256 modular doublings on the edge values of every
    class and 10^5 random values per class; here its constants and a sample of its (value, result) pairs against Python integers."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), "montform_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "montform_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr
    assert int(r.stdout.split("checked")[1].split()[0]) >= 600000
    kv = {}; samples = []
    for line in r.stdout.split("\n"):
        w = line.split()
        if len(w) == 2 and w[1].startswith("0x"):
            kv[w[0]] = int(w[1], 16)
        if w and w[0] == "sample":
            samples.append((int(w[1], 16), int(w[3], 16)))
    for i in range(8):      # the fixed constants re-derived from r
        assert kv[f"c{i}"] == (1 << (256 + 32 * i)) % R_MOD
    assert kv["mu"] == (1 << 317) // R_MOD
    for rb in (84, 65, 64):
        assert kv[f"neg{rb}"] == ((R_MOD - (1 << rb)) << 256) % R_MOD
    assert len(samples) >= 100
    edges = {0, 1, (1 << 21) - 1, (1 << 13) - 1, (1 << 8) - 1, 1 << 63, (1 << 64) - 1, 2**64 - 2**32, 2**64 - 2**32 + 1, 1 << 84, 1 << 65, 1 << 64,
             (1 << 128) - 1, R_MOD - 1, R_MOD - (1 << 84), R_MOD - (1 << 65), R_MOD - (1 << 64)}
    assert edges <= {v for v, _ in samples}, edges - {v for v, _ in samples}
    for v, m in samples:
        assert m == (v << 256) % R_MOD, hex(v)


@pytest.mark.parametrize("mode", [1, 0])
def test_direct_cell_map_is_the_complement_of_the_records(h2w, h2w_api, consts, mode):
    """What the ranged pass converts: the cells marked direct are exactly those no block record covers."""
    ko, kh = consts
    for args in [dict(degree_bits=6, num_queries=2), dict(degree_bits=7, num_queries=3, rate_bits=2, lookup_bits=13)]:
        plan = h2w_api.Plan(h2w.fibonacci_shape(args.pop("degree_bits"), args.pop("num_queries"), hash_mode=mode, **args), kh)
        direct = np.unpackbits(plan.direct_cells(), bitorder="little")
        assert not direct[plan.num_cells:].any()
        direct = direct[:plan.num_cells].astype(bool)
        assert int(direct.sum()) == plan.num_cells - plan.num_record_cells
        rr = plan.record_ranges().astype(np.int64)
        assert len(rr) == plan.num_records and int(rr[:, 1].sum()) == plan.num_record_cells
        cover = np.zeros(plan.num_cells + 1, dtype=np.int64)
        np.add.at(cover, rr[:, 0], 1); np.add.at(cover, rr[:, 0] + rr[:, 1], -1)
        cover = np.cumsum(cover)[:plan.num_cells]
        assert cover.max() == 1, "records overlap"
        assert ((cover == 0) == direct).all()
        plan.close()


def test_form_option_without_a_device(h2w, h2w_api, consts):
    """The option's values are checked wherever the plan lives."""
    ko, kh = consts
    plan = h2w_api.Plan(h2w.fibonacci_shape(5, 1, hash_mode=0), kh)
    with pytest.raises(h2w_api.H2WError, match="OUTPUT_FORM"):
        plan.configure(h2w_api.OPT_OUTPUT_FORM, 2)
    plan.set_output_form(h2w_api.FORM_CANONICAL)
    plan.close()
