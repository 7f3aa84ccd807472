// One 16-byte group of one stripe: the tile walk of the batched repair kernels, shared as TEXT by
// gf_repair.hip and gf_varlen.hip. NOT a header to include at file scope and without an include
// guard: each kernel includes it inside its column-block loop, after the tail branch. As an
// inlined function the same statements compiled to other code in gf_repair.hip's kernels (one more
// VGPR, other SGPR spills), and those kernels are pinned by profiles/repair.
// Expects in scope: MT (output rows per tile = min(4, m_pad), so m_pad is a multiple of MT and every
// tile row has a table column; rows past a pattern's e hold zero maps and a 0 out pointer), the
// stripe's RepairView `v`, its table block `tb`, `k`, `m_pad` and the lane's group index `g`; every row
// of the stripe 16-byte aligned. The lane walks the tiles, re-reading its own 16 bytes of the k inputs
// per tile; a tile whose out pointers are all 0 is skipped by one scalar branch. kRing input rows are
// kept in flight by a static register ring, consumed in pairs.
    const int64_t off = g * 16;
    for (int i0 = 0; i0 < m_pad; i0 += MT) {
      uint64_t op[MT], any = 0;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        op[i] = v.out[i0 + i];
        any |= op[i];
      }
      if (!any) continue;  // (wave-uniform: this stripe has fewer erasures than the widest pattern)

      uint32_t acc[MT][4];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[i][w] = 0;

      u32x4 ring[kRing];
#pragma unroll
      for (int u = 0; u < kRing; ++u)
        if (u < k) ring[u] = ld16<true>(row_vec(v.in[u], off));

      for (int j0 = 0; j0 < k; j0 += kRing) {
#pragma unroll
        for (int u = 0; u < kRing; u += 2) {
          const int j = j0 + u;
          if (j + 1 < k) {
            const u32x4 x0 = ring[u], x1 = ring[u + 1];
            if (j + kRing < k) ring[u] = ld16<true>(row_vec(v.in[j + kRing], off));
            if (j + 1 + kRing < k) ring[u + 1] = ld16<true>(row_vec(v.in[j + 1 + kRing], off));
            const auto t0 = tb + (size_t(j) * m_pad + i0) * kPermStride;
            const auto t1 = t0 + size_t(m_pad) * kPermStride;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const Sel s0 = make_sel(x0[w]);
              const Sel s1 = make_sel(x1[w]);
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[i][w] = mac_pair(acc[i][w], t0 + i * kPermStride, s0, t1 + i * kPermStride, s1);
            }
          } else if (j < k) {
            const u32x4 x = ring[u];
            const auto t = tb + (size_t(j) * m_pad + i0) * kPermStride;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const Sel s = make_sel(x[w]);
#pragma unroll
              for (int i = 0; i < MT; ++i) acc[i][w] = mac_map(acc[i][w], t + i * kPermStride, s);
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
        if (op[i]) st16<true>(row_vec_w(op[i], off), u32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]});
    }
