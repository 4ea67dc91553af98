"""GPU: a context's device workspaces after they were grown and then reused at
a smaller size.

Every entry that ends in the i8 MFMA key-switch GEMM keeps its digits, bodies
and result in a buffer of the context that one helper grows on demand. For
each of five entries, one TOY context runs 16 rows, then 130 rows (past the
128-row ciphertext block, a grow), then the first 16 rows again; the three
outputs equal, word for word, those of fresh contexts given the same keys and
inputs. Equality is exact: these paths draw no randomness, and the partial
sums of the GEMM's K split meet by 64-bit integer atomics, whose order does
not matter."""
import numpy as np
import pytest
import torch

from fheicp.engine import Engine
from fheicp.params import TOY

pytestmark = pytest.mark.gpu

U = np.uint64
SMALL, LARGE = 16, 130
BIG = TOY.k * TOY.N
N1 = (TOY.k + 1) * TOY.N


def dev_u64(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U).view(np.int64)).to(eng.device)


def words(rng, *shape):
    return rng.integers(0, 2 ** 64, shape, dtype=U)


def check_regrow(make, run):
    """make() -> a context with its keys in place; run(eng, rows) -> the
    entry's output for the first `rows` rows, as a host array."""
    eng = make()
    got = [run(eng, SMALL), run(eng, LARGE), run(eng, SMALL)]
    eng.close()
    want = {}
    for rows in (SMALL, LARGE):
        fresh = make()
        want[rows] = run(fresh, rows)
        fresh.close()
    for g, rows in zip(got, (SMALL, LARGE, SMALL)):
        np.testing.assert_array_equal(g, want[rows])


def test_keyswitch_regrow(need_gpu):
    ct = words(np.random.default_rng(1), LARGE, BIG + 1)

    def make():
        eng = Engine(TOY, 0)
        eng.keygen(77)
        return eng

    check_regrow(make, lambda eng, rows: eng.keyswitch(dev_u64(eng, ct[:rows])).cpu().numpy())


def test_pack_regrow(need_gpu):
    beta, lv = 4, 3
    rng = np.random.default_rng(2)
    pk = words(rng, BIG * lv * N1)
    ct = words(rng, LARGE, BIG + 1)

    def make():
        eng = Engine(TOY, 0)
        eng.import_pack_key(beta, lv, pk)
        return eng

    check_regrow(make, lambda eng, rows: eng.pack(dev_u64(eng, ct[:rows]), rows).cpu().numpy().reshape(-1, TOY.N))


def test_bridge_regrow(need_gpu):
    beta, lv = 4, 3
    rng = np.random.default_rng(3)
    bk = words(rng, BIG, lv, BIG + 1)
    ct = words(rng, LARGE, BIG + 1)

    def make():
        eng = Engine(TOY, 0)
        eng.import_bridge_key(beta, lv, bk)
        return eng

    check_regrow(make, lambda eng, rows: eng.bridge(dev_u64(eng, ct[:rows])).cpu().numpy())


def test_linear_ggsw_regrow(need_gpu):
    """D = N: one document per GLWE, so the rows are the GEMM's rows."""
    beta, lv, D = 4, 2, TOY.N
    rng = np.random.default_rng(4)
    ggsw = words(rng, (TOY.k + 1) * lv, TOY.k + 1, TOY.N)
    glwe = words(rng, LARGE, N1)

    def run(eng, rows):
        docs8 = eng.pack_docs_glwe(dev_u64(eng, glwe[:rows]), rows, D, beta, lv)
        return eng.linear_ggsw(dev_u64(eng, ggsw), beta, lv, docs8, rows, D, 5).cpu().numpy()

    check_regrow(lambda: Engine(TOY, 0), run)


def test_linear_queries_regrow(need_gpu):
    """The plane workspace this entry shares with fhe_linear_query_batch grows
    with the queries, not the rows: Q = 1 at 16 rows, Q = 3 at 130."""
    D = 5
    rng = np.random.default_rng(5)
    ct_q = words(rng, 3 * D, BIG + 1)
    dq = rng.integers(-128, 128, (LARGE, D))
    w = rng.integers(-3, 4, D)

    def run(eng, rows):
        Qn = 1 if rows == SMALL else 3
        docs8 = eng.pack_docs(eng.to_dev(dq[:rows]))
        return eng.linear_queries(dev_u64(eng, ct_q[:Qn * D]), Qn, docs8, rows, D, w, [7, -2, 11][:Qn]).cpu().numpy()

    check_regrow(lambda: Engine(TOY, 0), run)
