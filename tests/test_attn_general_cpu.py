"""Host-side refusals of ae_attn_fwd_bf16's general path (no GPU): attn_kernel of attention.hip addresses one (batch, head) image of K / V through
a buffer descriptor and 32-bit byte offsets, so the library refuses an image whose byte extent ((Nk - 1) row_stride + D) * 2 reaches 2^31 instead of
reading wrapped addresses.  Every call here is over the limit and returns before any launch: this machine has no GPU, a launch would come back as
a launch error (or not at all), and the buffer behind the pointers is a few bytes."""
import pytest
import torch

UNSUPPORTED = -3            # AE_ERR_UNSUPPORTED (csrc/common.hpp)
LIM = 1 << 30               # elements: 2^31 bytes of bf16


def _call(D, Nk=2, k_sn=None, v_sn=None, seg2=None):
    """ae_attn_fwd_bf16 on one (batch, head) with one query row; seg2 = (Nk2, k2_sn, v2_sn).  Strides default to contiguous rows."""
    from anyedit_amd import _lib
    L = _lib.lib
    p = torch.zeros(64, dtype=torch.bfloat16).data_ptr()
    k_sn, v_sn = k_sn or D, v_sn or D
    if seg2:
        Nk2, k2_sn, v2_sn = seg2
        s2 = (p, p, Nk2, 0, 0, k2_sn, 0, 0, v2_sn, p)
    else:
        s2 = (None, None, 0, 0, 0, 0, 0, 0, 0, None)
    rc = L.ae_attn_fwd_bf16(p, p, p, p, 1, 1, 1, Nk, D, 0, 0, D, 0, 0, k_sn, 0, 0, v_sn, 0, 0, D, D ** -0.5, None, None, 0, 0, None, None, 0,
                            *s2, None, None, None)
    return rc, L.ae_last_error()


# d = 64: attention.hip alone; d = 40: attention_fast.hip declines the same image first, then the general path must refuse it too
@pytest.mark.parametrize("D", [64, 40])
@pytest.mark.parametrize("which", ["k", "v", "k_many_rows", "k2", "v2"])
def test_kv_image_past_32_bit_offsets_is_refused(D, which):
    reach = LIM - D             # (Nk - 1) * stride + D == 2^30 elements with Nk = 2: the extent REACHES 2^31 bytes
    assert reach % 8 == 0
    args = dict(k=dict(k_sn=reach), v=dict(v_sn=reach), k_many_rows=dict(Nk=1025, k_sn=1 << 20),
                k2=dict(seg2=(2, reach, D)), v2=dict(seg2=(2, D, reach)))[which]
    rc, msg = _call(D, **args)
    assert rc == UNSUPPORTED, (rc, msg)
    assert b"ae_attn_fwd_bf16" in msg and b"2^31" in msg, msg


def test_the_refusal_names_the_sizes():
    rc, msg = _call(64, Nk=1025, k_sn=1 << 20)
    assert rc == UNSUPPORTED and b"Nk=1025" in msg and b"k_sn=1048576" in msg and b"head_dim 64" in msg, msg
