"""bm_bucket_masks_device on the GPU: the masks of a run of counters against the host form, the counter word advancing by
one per launch, and a recorded graph drawing the masks of consecutive counters at its replays.
Needs an MI355X: `pytest -m gpu`."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def _signed(x):
  x &= U64
  return x - (1 << 64) if x >= (1 << 63) else x


def _counter(value):
  return torch.tensor([_signed(value)], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("n,s", [(1, 1), (2, 1), (2, 2), (5, 2), (11, 2), (11, 3), (25, 2), (25, 3), (63, 2), (64, 1), (64, 3),
                                 (64, 64)])
def test_device_masks_equal_host_masks_over_a_run_of_counters(bm, n, s):
  for seed, start in ((0, 0), (12345, 2 ** 32 - 3), (U64, U64 - 2)):   # (the last run wraps the counter around)
    counter = _counter(start)
    got = [bm.gars.bucket_masks_device(n, s, seed, counter) for _ in range(6)]
    assert counter.item() == _signed(start + 6)                          # advanced by one per launch
    for i, masks in enumerate(got):
      assert masks.dtype == torch.int64 and masks.shape == (64,) and masks.is_cuda
      want = bm.gars.bucket_masks_host(n, s, seed, (start + i) & U64)
      assert torch.equal(masks.cpu(), want), (n, s, seed, start + i)


def test_out_tensor_and_refusals(bm):
  counter, out = _counter(0), torch.full((64,), -1, dtype=torch.int64, device=DEV)
  assert bm.gars.bucket_masks_device(11, 2, 0, counter, out=out) is out
  assert [w & U64 for w in out.tolist()] == [0x60, 0x9, 0x410, 0x6, 0x300, 0x80] + [0] * 58
  with pytest.raises(ValueError):
    bm.gars.bucket_masks_device(11, 12, 0, counter)
  with pytest.raises(ValueError):
    bm.gars.bucket_masks_device(11, 2, 0, torch.zeros(1, dtype=torch.int64))       # a host counter
  with pytest.raises(ValueError):
    bm.gars.bucket_masks_device(11, 2, 0, torch.zeros(1, dtype=torch.int32, device=DEV))
  assert counter.item() == 1


def test_graph_replays_draw_consecutive_counters(bm):
  from byzantinemomentum_amd.graphs import GraphedCall
  n, s, seed, warmup = 25, 2, 99, 2
  counter, out = _counter(0), torch.zeros(64, dtype=torch.int64, device=DEV)
  call = GraphedCall(lambda: bm.gars.bucket_masks_device(n, s, seed, counter, out=out), warmup=warmup)
  torch.cuda.synchronize()
  first = int(counter.item())
  assert first == warmup          # the warm-up ran the kernel; the recording itself launched nothing
  seen = []
  for i in range(4):
    masks = call()
    torch.cuda.synchronize()
    assert masks is out
    seen.append(masks.cpu().clone())
    assert counter.item() == first + i + 1
  for i, masks in enumerate(seen):
    assert torch.equal(masks, bm.gars.bucket_masks_host(n, s, seed, first + i)), i
  assert len({tuple(m.tolist()) for m in seen}) == 4
