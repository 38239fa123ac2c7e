"""Mirror of AnyEdit_Collection/other_modules/prompt2prompt/seq_aligner.py: the token mappers of the replace and refine controllers.  Host code; the
outputs equal the reference's exactly (integers and the values 0, 1 and 1 / n).  The tokenizer is passed in (`encode(text)` with the start and end
tokens, `decode([id])` of one piece), as everywhere in this package."""
import numpy as np
import torch

_LEFT, _UP, _DIAG, _STOP = 1, 2, 3, 4


def global_align(x, y, gap=0, match=1, mismatch=-1):
    """seq_aligner.py:61-77: Needleman-Wunsch scores and moves; ties prefer a gap in x (left), then a gap in y (up), then the diagonal"""
    nx, ny = len(x), len(y)
    score = np.zeros((nx + 1, ny + 1), dtype=np.int32)
    score[0, 1:] = (np.arange(ny) + 1) * gap
    score[1:, 0] = (np.arange(nx) + 1) * gap
    move = np.zeros((nx + 1, ny + 1), dtype=np.int32)
    move[0, 1:] = _LEFT
    move[1:, 0] = _UP
    move[0, 0] = _STOP
    for i in range(1, nx + 1):
        for j in range(1, ny + 1):
            left, up = score[i, j - 1] + gap, score[i - 1, j] + gap
            diag = score[i - 1, j - 1] + (match if x[i - 1] == y[j - 1] else mismatch)
            best = max(left, up, diag)
            score[i, j] = best
            move[i, j] = _LEFT if best == left else _UP if best == up else _DIAG
    return score, move


def get_aligned_sequences(x, y, move):
    """seq_aligner.py:80-105: int64 [len(y), 2] pairs (token of y, its token of x or -1 for an insertion)"""
    i, j = len(x), len(y)
    pairs = []
    while i > 0 or j > 0:
        m = move[i, j]
        if m == _DIAG:
            i, j = i - 1, j - 1
            pairs.append((j, i))
        elif m == _LEFT:
            j -= 1
            pairs.append((j, -1))
        elif m == _UP:
            i -= 1
        else:
            break
    pairs.reverse()
    return torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)


def get_mapper(x, y, tokenizer, max_len=77):
    """seq_aligner.py:108-119: (mapper int64 [max_len], alphas fp32 [max_len]); mapper[j] = the token of x behind token j of y (-1: inserted),
    alphas[j] = 0 for an inserted token; past y's tokens the mapper continues len(y) + 0, 1, ..."""
    x_seq, y_seq = tokenizer.encode(x), tokenizer.encode(y)
    _, move = global_align(x_seq, y_seq)
    pairs = get_aligned_sequences(x_seq, y_seq, move)
    n = pairs.shape[0]
    alphas = torch.ones(max_len)
    alphas[:n] = pairs[:, 1].ne(-1).float()
    mapper = torch.zeros(max_len, dtype=torch.int64)
    mapper[:n] = pairs[:, 1]
    mapper[n:] = len(y_seq) + torch.arange(max_len - len(y_seq))
    return mapper, alphas


def get_refinement_mapper(prompts, tokenizer, max_len=77):
    """seq_aligner.py:122-129"""
    res = [get_mapper(prompts[0], p, tokenizer, max_len) for p in prompts[1:]]
    return torch.stack([m for m, _ in res]), torch.stack([a for _, a in res])


def get_word_inds(text, word_place, tokenizer):
    """seq_aligner.py:132-150: token indices (1-based behind the start token) of the word(s) `word_place` (an index into text.split(' ') or a word)"""
    words = text.split(" ")
    if type(word_place) is str:
        word_place = [i for i, w in enumerate(words) if w == word_place]
    elif type(word_place) is int:
        word_place = [word_place]
    out = []
    if len(word_place) > 0:
        pieces = [tokenizer.decode([t]).strip("#") for t in tokenizer.encode(text)][1:-1]
        seen, ptr = 0, 0
        for i, piece in enumerate(pieces):
            seen += len(piece)
            if ptr in word_place:
                out.append(i + 1)
            if seen >= len(words[ptr]):
                ptr += 1
                seen = 0
    return np.array(out)


def get_replacement_mapper_(x, y, tokenizer, max_len=77):
    """seq_aligner.py:153-185: fp32 [max_len, max_len]; identity outside the replaced words, a block of 1 (equal piece counts) or 1 / n (n target
    pieces) between a replaced word's source and target pieces"""
    wx, wy = x.split(" "), y.split(" ")
    if len(wx) != len(wy):
        raise ValueError(f"attention replacement edit can only be applied on prompts with the same length but prompt A has {len(wx)} words and "
                         f"prompt B has {len(wy)} words.")
    changed = [i for i in range(len(wy)) if wy[i] != wx[i]]
    src = [get_word_inds(x, i, tokenizer) for i in changed]
    tgt = [get_word_inds(y, i, tokenizer) for i in changed]
    mapper = np.zeros((max_len, max_len))
    i = j = cur = 0
    while i < max_len and j < max_len:
        if cur < len(src) and src[cur][0] == i:
            s, t = src[cur], tgt[cur]
            if len(s) == len(t):
                mapper[s, t] = 1
            else:
                for jt in t:
                    mapper[s, jt] = 1 / len(t)
            cur += 1
            i += len(s)
            j += len(t)
        elif cur < len(src):
            mapper[i, j] = 1
            i += 1
            j += 1
        else:
            mapper[j, j] = 1
            i += 1
            j += 1
    return torch.from_numpy(mapper).float()


def get_replacement_mapper(prompts, tokenizer, max_len=77):
    """seq_aligner.py:189-195"""
    return torch.stack([get_replacement_mapper_(prompts[0], p, tokenizer, max_len) for p in prompts[1:]])
