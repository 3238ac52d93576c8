// cbev_expand.inc -- the frame-stack expansion kernels, included twice by cbev.hip:
// once with one head for all envs (k_expand_semantic, k_expand_semantic_bits,
// k_expand_gray: `int head`), once with a head per env (the same names + _heads:
// `const uint8_t* heads`, cbev_expand_obs_heads). The includer defines
//   CBEV_EXPAND_KERNEL(name)  the kernel's name
//   CBEV_HEAD_PARAM           the head parameter's declaration
//   CBEV_HEAD_OF_ENV          nothing, or the statement that defines `head` for env e
//                             of this thread iteration: heads[e] reduced modulo F, so
//                             no slot computed from it lies outside the ring
//   CBEV_SLOT(x)              x modulo F for 0 <= x < 3 F: `%` where the head is a kernel
//                             argument (scalar arithmetic), compares and subtractions where
//                             it is per thread (a division there costs the VALU-bound
//                             kernels 2 %: DESIGN.md, "Per-env frame-stack heads")
// Both forms are this one text, so the global-head kernels compile to what they
// were before the per-env form existed. The kernels' comments are in cbev.hip.

template <int FUSE, typename T, int V>
__global__ __launch_bounds__(256) void CBEV_EXPAND_KERNEL(k_expand_semantic)(const uint8_t* __restrict__ ring, int n, int F, CBEV_HEAD_PARAM, int C,
                                                         int vidx, int SS, Lut16 lut, T* __restrict__ out) {
  const int nv = SS / V;
  const int Cout = FUSE == 0 ? F * C : (FUSE == 1 ? C + 2 : C);
  const int64_t total = (int64_t)n * nv;
  for (int64_t q = blockIdx.x * 256ll + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t e = q / nv;
    CBEV_HEAD_OF_ENV
    const int64_t p = (q - e * nv) * V;
    T* o = out + e * Cout * (int64_t)SS + p;
    T vals[V];
    if (FUSE == 0) {
      for (int f = 0; f < F; ++f) {  // oldest -> newest
        const int slot = CBEV_SLOT(head + 1 + f);
        uint32_t m[V];
        load_masks<V>(ring + ((int64_t)slot * n + e) * SS + p, lut, m);
        for (int c = 0; c < C; ++c) {
#pragma unroll
          for (int k = 0; k < V; ++k) vals[k] = (T)((m[k] >> c) & 1);
          store_nt<T, V>(o + (int64_t)(f * C + c) * SS, vals);
        }
      }
    } else {
      uint32_t m0[V], m1[V], m2[V];  // newest, newest-1, newest-2
      load_masks<V>(ring + ((int64_t)head * n + e) * SS + p, lut, m0);
      load_masks<V>(ring + ((int64_t)CBEV_SLOT(head - 1 + F) * n + e) * SS + p, lut, m1);
      load_masks<V>(ring + ((int64_t)CBEV_SLOT(head - 2 + 2 * F) * n + e) * SS + p, lut, m2);
      int oc = 0;
      for (int c = 0; c < C; ++c) {  // static channels of the newest frame
        if (c == vidx) continue;
#pragma unroll
        for (int k = 0; k < V; ++k) vals[k] = (T)((m0[k] >> c) & 1);
        store_nt<T, V>(o + (int64_t)(oc++) * SS, vals);
      }
      if (FUSE == 1) {
#pragma unroll
        for (int k = 0; k < V; ++k) vals[k] = (T)((m0[k] >> vidx) & 1);
        store_nt<T, V>(o + (int64_t)oc * SS, vals);
#pragma unroll
        for (int k = 0; k < V; ++k) vals[k] = (T)((m1[k] >> vidx) & 1);
        store_nt<T, V>(o + (int64_t)(oc + 1) * SS, vals);
#pragma unroll
        for (int k = 0; k < V; ++k) vals[k] = (T)((m2[k] >> vidx) & 1);
        store_nt<T, V>(o + (int64_t)(oc + 2) * SS, vals);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {  // float32 in the reference's order, clipped, then converted
          float acc = 0.0f;
          acc += 1.0f * (float)((m0[k] >> vidx) & 1);
          acc += 0.5f * (float)((m1[k] >> vidx) & 1);
          acc += 0.25f * (float)((m2[k] >> vidx) & 1);
          vals[k] = (T)fminf(fmaxf(acc, 0.0f), 1.0f);
        }
        store_nt<T, V>(o + (int64_t)oc * SS, vals);
      }
    }
  }
}

template <int FUSE, int V>
__global__ __launch_bounds__(256) void CBEV_EXPAND_KERNEL(k_expand_semantic_bits)(const uint8_t* __restrict__ ring, int n, int F, CBEV_HEAD_PARAM,
                                                              int C, int vidx, int SS, Lut16 lut,
                                                              uint8_t* __restrict__ out) {
  __shared__ uint32_t idset[16];
  if (threadIdx.x < 16) {
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t |= ((lut.v[i] >> threadIdx.x) & 1u) << i;
    idset[threadIdx.x] = t;
  }
  __syncthreads();
  const int PB = (SS + 7) >> 3;
  const int nv = (SS + V - 1) / V;
  const int Cout = FUSE == 0 ? F * C : C + 2;
  const int64_t total = (int64_t)n * nv;
  for (int64_t q = blockIdx.x * 256ll + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t e = q / nv;
    CBEV_HEAD_OF_ENV
    const int j = (int)(q - e * nv);
    const int p = j * V, left = SS - p;
    const uint32_t valid = left >= V ? 0xffffffffu : (1u << left) - 1u;
    uint8_t* o = out + e * Cout * (int64_t)PB + j * (V / 8);
    uint32_t id[V];
    if (FUSE == 0) {
      for (int f = 0; f < F; ++f) {  // oldest -> newest
        const int slot = CBEV_SLOT(head + 1 + f);
        load_ids_b<V>(ring + ((int64_t)slot * n + e) * SS + p, left, id);
        for (int c = 0; c < C; ++c) store_bits<V>(o + (int64_t)(f * C + c) * PB, plane_bits<V>(id, idset[c], valid));
      }
    } else {
      const uint32_t vset = idset[vidx];
      load_ids_b<V>(ring + ((int64_t)CBEV_SLOT(head - 1 + F) * n + e) * SS + p, left, id);
      const uint32_t v1 = plane_bits<V>(id, vset, valid);
      load_ids_b<V>(ring + ((int64_t)CBEV_SLOT(head - 2 + 2 * F) * n + e) * SS + p, left, id);
      const uint32_t v2 = plane_bits<V>(id, vset, valid);
      load_ids_b<V>(ring + ((int64_t)head * n + e) * SS + p, left, id);
      int oc = 0;
      for (int c = 0; c < C; ++c) {  // static channels of the newest frame
        if (c == vidx) continue;
        store_bits<V>(o + (int64_t)(oc++) * PB, plane_bits<V>(id, idset[c], valid));
      }
      store_bits<V>(o + (int64_t)oc * PB, plane_bits<V>(id, vset, valid));
      store_bits<V>(o + (int64_t)(oc + 1) * PB, v1);
      store_bits<V>(o + (int64_t)(oc + 2) * PB, v2);
    }
  }
}

template <bool RAW, int V>
__global__ __launch_bounds__(256) void CBEV_EXPAND_KERNEL(k_expand_gray)(const uint8_t* __restrict__ ring, int n, int F, CBEV_HEAD_PARAM, int SS,
                                                     Lut16 lut, uint8_t* __restrict__ out) {
  const int nv = SS / V;
  const int64_t total = (int64_t)n * F * nv;
  for (int64_t q = blockIdx.x * 256ll + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
    const int64_t pv = q % nv;
    const int64_t ef = q / nv;
    const int f = (int)(ef % F);
    const int64_t e = ef / F;
    CBEV_HEAD_OF_ENV
    const int slot = CBEV_SLOT(head + 1 + f);
    const uint8_t* src = ring + ((int64_t)slot * n + e) * SS + pv * V;
    uint8_t* dst = out + (e * F + f) * (int64_t)SS + pv * V;
    if (V == 16) {
      uint4 ids = *(const uint4*)src;
      if (!RAW) {
        uint32_t in[4] = {ids.x, ids.y, ids.z, ids.w}, o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          o[k] = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[k] |= (lut.v[(in[k] >> (8 * j)) & 15] & 255u) << (8 * j);
        }
        ids = make_uint4(o[0], o[1], o[2], o[3]);
      }
      nt_u4 x = {ids.x, ids.y, ids.z, ids.w};
      __builtin_nontemporal_store(x, (nt_u4*)dst);
    } else {
      dst[0] = RAW ? src[0] : (uint8_t)lut.v[src[0] & 15];
    }
  }
}
