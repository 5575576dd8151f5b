"""The in-process hand-off from a pooled engine to the sample store, in a process of its own (the store wants torch's HIP runtime
loaded before the library): run by tests/test_gpu_start_pool.py as `python -m tests.start_pool_store_check OUT.json`
(tests/fresh_process.py)."""
import numpy as np
import torch  # noqa: F401  (its HIP runtime first: link.require_torch_runtime)

from ataxxzero_amd import link
from tests import engine_harness as eh
from tests import fresh_process
from tests import start_pool_fixtures as spf


def check_records_enter_the_store_with_their_own_masks():
    pool, net = spf.entries(), eh.net()
    e = spf.pooled_engine(pool, 6, 8)
    words = np.zeros(0, np.uint32)
    for _ in range(40):
        e.run(net, 100, link.DTYPE_F32)
        words = np.concatenate([words, eh.staged(e)])
        if len(list(link.records(words))) >= 8:
            break
    recs = list(link.records(words))
    assert len(recs) >= 8
    masks = e.record_blockers(words)
    assert [int(m) for m in masks] == [pool[r.uid % 4][2] for r in link.records(words, markers=True)]
    assert len({int(m) for m in masks}) >= 3
    store = link.SampleStore(64, 64 * 400, 64 * 400 * 32)
    store.add_records(words, masks)
    assert [int(m) for m in store.game_blockers()] == [pool[r.uid % 4][2] for r in recs]
    assert store.counts()["games"] == len(recs)
    for bad in (masks[:-1], np.concatenate([masks, masks[:1]]), masks | np.uint64(1 << 49)):
        try:
            store.add_records(words, bad)
        except link.AzhError:
            pass
        else:
            raise AssertionError("a wrong mask array was taken")
    assert store.counts()["games"] == len(recs)                  # a refused call adds nothing
    # a game's stones never stand on its own walls, so the masks of another order are refused where they collide — and the
    # aux path (owners from the last move under the game's own walls) takes the right ones
    aux = link.SampleStore(64, 64 * 400, 64 * 400 * 32)
    aux.add_records(words, masks, aux=True)
    assert aux.counts()["games"] == len(recs)
    store.close()
    aux.close()


CHECKS = [check_records_enter_the_store_with_their_own_masks]

if __name__ == "__main__":
    fresh_process.main(CHECKS)
