"""The bias gradient of the streaming T5 attention (attn_rlong_dkdv_kernel of csrc/attention_long.hip) the way the kernel forms it, in
fp32 torch on one item, and three planted defects of that structure.  Not a test module: tests/test_attention_rel_long_ref.py checks
on the CPU that the drel comparison of tests/attention_ref.py rejects each of them, tests/test_attention_rel_long_gpu.py takes the
bound of the whole call from here.

The structure.  A dK / dV workgroup owns the 128 keys of one key block and streams the queries in 64-row chunks; an element (query,
key) of the fp32 dS goes to the diagonal key - query + seq - 1, where `query` is the chunk's first row r0 plus the row inside the
chunk; the diagonals are summed per bucket and every (item, key block) stores one partial per bucket and head; the partials are
added in (item, key block) order.  Rows and keys at or beyond seq add nothing.

The defects (drel of one head of one item wrong in ONE way):
  missing_key_block      : the partial of one key block is not added
  diag_without_chunk_row : the diagonal of the elements of one 64-row chunk is taken with the row inside the chunk instead of r0 + row
                           (diagonals behind the table are dropped)
  dead_rows_admitted     : the rows seq .. (seq rounded up to 32) - 1 of the last chunk are admitted; a kernel that does not zero them
                           holds copies of row seq - 1 there (the loads are clamped to the last row), so each adds that row's dS at
                           its own diagonal
The bound of the call (drel_call_bound): the reference's per-item bounds (attention_ref.backward_reference: the fp32 dS's own error
plus an fp32 summation term) summed over the items, plus
  2 (batch * ceil(seq / 128) + 2) e * sum |dS|   the fp32 error of adding that many partials (reduce_partials' tree and the add into drel),
  2^-41 * (elements of the bucket)               the fixed point: every term is rounded once to 2^-40 units (half a unit each at most;
                                                 a pre-summed value of up to four elements rounds once, so this counts too many).
"""
import math

import torch

import attention_ref as R

KEY_BLOCK, Q_CHUNK = 128, 64
DEFECTS = ("missing_key_block", "diag_without_chunk_row", "dead_rows_admitted")


def emulated_ds(it, out_in, lse_in):
    """fp32 dS [H][Tq][Tk] with the rounding points of attention_ref.emulate_backward"""
    Q, K, V, O, dO = (x.float().permute(1, 0, 2) for x in (it.q, it.k, it.v, out_in, it.dout))
    sl2 = torch.tensor(it.scale * R.LOG2E, dtype=torch.float32)
    s2 = (Q @ K.transpose(1, 2)) * sl2 + it.bias().float() * torch.tensor(R.LOG2E, dtype=torch.float32)
    lse2 = lse_in.float() * torch.tensor(R.LOG2E, dtype=torch.float32)
    p = torch.exp2(s2 - lse2[..., None])
    dP = dO @ V.transpose(1, 2)
    if it.drop is not None:
        dP = dP * it.drop.float()
    return p * (dP - (dO * O).sum(-1)[..., None])


def applies(defect, seq):
    if defect == "missing_key_block":
        return seq > 1                     # (one token: p = 1 and dS = 0 exactly)
    if defect == "diag_without_chunk_row":
        return seq > Q_CHUNK
    if defect == "dead_rows_admitted":
        return seq > 1 and seq % 32 != 0
    raise ValueError(defect)


def drel_streamed(it, out_in, lse_in, defect=None, head=0, where=-1):
    """drel fp32 [buckets][H] of one item, summed as the kernel sums it.  defect: one of DEFECTS on head `head`; where: the key block
    (missing_key_block) or the query chunk (diag_without_chunk_row) it sits in, negative: counted from the last"""
    dS = emulated_ds(it, out_in, lse_in)
    H, T = it.H, it.Tq
    nb, bucket = it.nbuckets(), it.rel_bucket.long()
    nkb, nch = -(-T // KEY_BLOCK), -(-T // Q_CHUNK)
    where_kb, where_c = where % nkb, (where % (nch - 1) + 1 if nch > 1 else 0)          # a chunk with r0 > 0
    total = torch.zeros(nb, H, dtype=torch.float32)
    for kb in range(nkb):
        keys = torch.arange(kb * KEY_BLOCK, min(T, (kb + 1) * KEY_BLOCK))
        part = torch.zeros(nb, H, dtype=torch.float32)
        for c in range(nch):
            r0 = c * Q_CHUNK
            rows = torch.arange(r0, min(T, r0 + Q_CHUNK))
            blk = dS[:, rows][:, :, keys]
            diag = keys[None, :] - rows[:, None] + T - 1
            for h in range(H):
                d, x = diag, blk[h]
                if defect == "diag_without_chunk_row" and h == head and c == where_c:
                    d = diag + r0
                    keep = d <= 2 * T - 2
                    d, x = d[keep], x[keep]
                part[:, h].index_add_(0, bucket[d.flatten()], x.flatten())
            if defect == "dead_rows_admitted" and c == nch - 1:
                for r in range(T, -(-T // 32) * 32):
                    d = keys - r + T - 1
                    keep = d >= 0
                    part[:, head].index_add_(0, bucket[d[keep]], dS[head, T - 1, keys][keep])
        if defect == "missing_key_block" and kb == where_kb:
            part[:, head] = 0.0
        total += part
    return total


def bucket_counts(it):
    """elements (query, key) of every bucket, float64 [buckets]"""
    T = it.Tq
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    idx = it.rel_bucket.long().to("cpu")[j - i + T - 1].flatten()
    return torch.zeros(it.nbuckets(), dtype=torch.float64).index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float64))


def drel_call_bound(refs, batch, seq, counts):
    """(ref, bound) [buckets][H] of a whole call from the items' backward references (see the module docstring)"""
    ref = sum(r["drel"][0] for r in refs)
    mag = sum(r["drel_mag"] for r in refs)
    nparts = batch * math.ceil(seq / KEY_BLOCK)
    bound = sum(r["drel"][1] for r in refs) + 2.0 * (nparts + 2) * R.EPS32 * mag + 2.0 ** -41 * counts.to(mag.device)[:, None]
    return ref, bound
