"""The 16x16x32 form of the plane GEMMs (umx.cpp_amd/csrc/gemm_planes*.h, GP_MFMA_K32 = 1) restated in numpy: which bytes of the
staged LDS image a lane's fragment read returns, which banks a read group touches, and where the two lane swaps in front of the
epilogue put an accumulator element.

The kernels' maps:
  staging   a plane tile sits in LDS as rows of 64 bytes (32 k of fp16) in four 16-byte chunks; chunk c of row r is stored at chunk
            c ^ ((r >> 2) & 3) of that row (the LDS-DMA lane that lands at row r, physical chunk p fetches logical chunk p ^ ((r >> 2) & 3))
  fragment  lane l of a wave reads, for 16-row block b of its tile, the 16 bytes at (16 b + (l & 15)) * 64 + (c ^ ((l >> 2) & 3)) * 16 with
            q = l >> 4, c = (q + 3) & 3: element j of the operand of v_mfma_f32_16x16x32_f16 (the instruction's k = 8 q + j) is row
            16 b + (l & 15), k = 8 c + j of the tile -- the same c for both operands, so the instruction sums every product of the 32 k
            once, the chunks in the order 3, 0, 1, 2
  banks     ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, {32-35, 44-47, 52-59},
            {36-43, 48-51, 60-63}: each must touch every bank once (c = q does not: measured as a 2-way conflict on every read)
  result    register j of a 16 x 16 block holds row 4 (l >> 4) + j, column l & 15
  swaps     for a 32 x 32 square, X = register j of block (bm, 0), Y = register j of block (bm, 1) (bm: 16-row half, second index: 16-column
            half): v_permlane16_swap(X, Y) then v_permlane32_swap(X, Y) leave X = register 8 bm + j and Y = register 8 bm + 4 + j of the
            32x32x16 result layout the epilogues index (register R holds row (R & 3) + 8 (R >> 2) + 4 (L >> 5), column L & 31)
No GPU: the kernels themselves are tested in tests/test_gpu_gemm_k32.py and tests/test_gpu_batch.py."""
import numpy as np

ROW_BYTES, CHUNK = 64, 16


def stage_tile(tile):
    """tile [rows][32] fp16 -> the LDS image as the LDS-DMA writes it: 1 KiB per wave instruction, lane L at row 16 g + L / 4, physical
    chunk L % 4, fetching logical chunk (L % 4) ^ ((L / 16) & 3) of that row."""
    rows = tile.shape[0]
    src = tile.view(np.uint8).reshape(rows, ROW_BYTES)
    lds = np.zeros(rows * ROW_BYTES, np.uint8)
    for g in range(rows // 16):
        for lane in range(64):
            r, p = 16 * g + (lane >> 2), lane & 3
            c = p ^ ((lane >> 4) & 3)
            assert ((lane >> 4) & 3) == ((r >> 2) & 3)
            lds[g * 1024 + lane * 16:g * 1024 + lane * 16 + 16] = src[r, c * CHUNK:(c + 1) * CHUNK]
    return lds


def k_chunk(lane):
    q = lane >> 4
    return (q + 3) & 3


def fragment_offset(block, lane):
    return (16 * block + (lane & 15)) * ROW_BYTES + (k_chunk(lane) ^ ((lane >> 2) & 3)) * CHUNK


# the lanes one pass of ds_read_b128 serves
READ_GROUPS = [[l + h for l in g] for h in (0, 32) for g in ([0, 1, 2, 3, 12, 13, 14, 15] + list(range(20, 28)),
                                                             list(range(4, 12)) + [16, 17, 18, 19, 28, 29, 30, 31])]


def test_fragment_read_hands_every_lane_its_row_and_k_chunk():
    rng = np.random.default_rng(3)
    # one 128-row A tile of a wave (8 blocks) and its 64-row B tile (4 blocks): the same addressing
    for rows in (128, 64):
        tile = rng.standard_normal((rows, 32)).astype(np.float16)
        lds = stage_tile(tile)
        for block in range(rows // 16):
            for lane in range(64):
                off = fragment_offset(block, lane)
                got = lds[off:off + 16].view(np.float16)
                k0 = 8 * k_chunk(lane)
                want = tile[16 * block + (lane & 15), k0:k0 + 8]
                assert (got.view(np.uint16) == want.view(np.uint16)).all(), (rows, block, lane)
    # the four lane groups l >> 4 of an instruction take the four chunks of the 32 k once each, and a row of A meets a row of B on the
    # same k whatever the two rows are: the chunk depends on l >> 4 alone
    assert sorted(k_chunk(16 * q) for q in range(4)) == [0, 1, 2, 3]
    assert all(k_chunk(lane) == k_chunk(lane & 48) for lane in range(64))


def test_the_product_of_permuted_fragments_is_the_product():
    """v_mfma_f32_16x16x32_f16 modelled as D[i][j] = sum over lane groups q and elements e of A_frag[lane (q, i)][e] B_frag[lane (q, j)][e]:
    with both fragments read through fragment_offset it is A B^T over all 32 k (small integers: exact in any order)."""
    rng = np.random.default_rng(6)
    A = rng.integers(-8, 9, (16, 32)).astype(np.float16)
    B = rng.integers(-8, 9, (16, 32)).astype(np.float16)
    la, lb = stage_tile(A), stage_tile(B)
    D = np.zeros((16, 16), np.float64)
    for q in range(4):
        for i in range(16):
            fa = la[fragment_offset(0, 16 * q + i):][:16].view(np.float16).astype(np.float64)
            for j in range(16):
                fb = lb[fragment_offset(0, 16 * q + j):][:16].view(np.float16).astype(np.float64)
                D[i, j] += fa @ fb
    assert (D == A.astype(np.float64) @ B.astype(np.float64).T).all()


def test_every_read_group_touches_64_distinct_banks():
    # one pass of ds_read_b128 serves 16 lanes x 16 bytes = 64 banks of 4 bytes
    assert sorted(l for g in READ_GROUPS for l in g) == list(range(64)) and all(len(g) == 16 for g in READ_GROUPS)
    for block in range(8):
        for group in READ_GROUPS:
            banks = []
            for lane in group:
                off = fragment_offset(block, lane)
                banks += [((off >> 2) + w) & 63 for w in range(4)]
            assert len(set(banks)) == 64, (block, group)


def permlane16_swap(x, y):
    """v_permlane16_swap_b32: the odd 16-lane rows of the first operand change places with the even rows of the second."""
    x, y = x.copy(), y.copy()
    for row in (0, 2):
        a, b = slice(16 * (row + 1), 16 * (row + 2)), slice(16 * row, 16 * (row + 1))
        x[a], y[b] = y[b].copy(), x[a].copy()
    return x, y


def permlane32_swap(x, y):
    """v_permlane32_swap_b32: lanes 32-63 of the first operand change places with lanes 0-31 of the second."""
    x, y = x.copy(), y.copy()
    x[32:], y[:32] = y[:32].copy(), x[32:].copy()
    return x, y


def test_two_lane_swaps_turn_four_16x16_blocks_into_the_32x32_register_layout():
    rng = np.random.default_rng(4)
    square = rng.standard_normal((32, 32)).astype(np.float32)
    lanes = np.arange(64)
    # the 16x16x32 results: block (bm, bn), register j, lane l
    blk = np.zeros((2, 2, 4, 64), np.float32)
    for bm in range(2):
        for bn in range(2):
            for j in range(4):
                blk[bm, bn, j] = square[16 * bm + 4 * (lanes >> 4) + j, 16 * bn + (lanes & 15)]
    got = np.zeros((16, 64), np.float32)
    for bm in range(2):
        for j in range(4):
            x, y = permlane16_swap(blk[bm, 0, j], blk[bm, 1, j])
            x, y = permlane32_swap(x, y)
            got[8 * bm + j], got[8 * bm + 4 + j] = x, y
    for reg in range(16):
        want = square[(reg & 3) + 8 * (reg >> 2) + 4 * (lanes >> 5), lanes & 31]
        assert (got[reg] == want).all(), reg
