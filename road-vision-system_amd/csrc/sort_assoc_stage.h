// One stage of the association of sort_associate_kernel (csrc/sort.hip),
// included in the kernel's body once per stage with `stage` a compile-time
// constant in scope: 0 = the reference's _associate (sort_tracker.py:182-210;
// BYTE: over the high detections), 1 = BYTE's second association.  Plain
// text inclusion, not a loop or a function: the plain instances then compile
// to the code they had before there was a second stage.
    const double thr = stage == 0 ? p.iou_thr : (double)RV_BYTE_SECOND_IOU;
    // the pairs of this stage (every pair in the plain instances)
    auto in_stage = [&](int t, int d) -> bool {
      if constexpr (!BYTE)
        return true;
      else
        return stage == 0 ? dcls[d] != 0 : (dcls[d] == 0 && elig[t] != 0 && trk_match[t] < 0);
    };
    if (T > 0 && D > 0) {
      if (BYTE && stage == 1) {  // stage 1's matches are visible, its count is read
        __syncthreads();
        if (tid == 0) s_cnt = 0;
        __syncthreads();
      }
      // qualifying pairs appended with one LDS atomic per wave (a ballot's
      // popcount), not one per pair; the append order does not matter (the
      // keys are sorted next and unique)
      // pair i = tid + kAssocThreads k is (i / D, i % D), stepped
      // incrementally (an integer division by the runtime D per pair was ~20
      // VALU, as much as the IoU itself)
      const int dt = kAssocThreads / D, dd = kAssocThreads - (kAssocThreads / D) * D;
      int pt = tid / D, pd = tid - (tid / D) * D;
      for (int i0 = 0; i0 < T * D; i0 += kAssocThreads) {
        const int i = i0 + tid;
        bool q = false;
        float v = 0.f;
        if (i < T * D && in_stage(pt, pd)) {
          v = iou_f32(tbox[pt], dbox[pd]);
          q = (double)v >= thr;
        }
        pt += dt;
        pd += dd;
        if (pd >= D) {
          pd -= D;
          ++pt;
        }
        const unsigned long long m = __ballot(q);
        if (m) {  // wave-uniform
          int base = 0;
          if (lane == 0) base = atomicAdd(&s_cnt, __popcll(m));
          base = __shfl(base, 0);
          if (q) {
            const int k = base + __popcll(m & ((1ull << lane) - 1ull));
            if (k < kKeyCap) keys[k] = ((uint64_t)(~__float_as_uint(v)) << 32) | (uint64_t)(uint32_t)i;
          }
        }
      }
      __syncthreads();
      RV_PH(1);  // IoU pairs
      const int cnt = s_cnt;
      if (cnt <= kKeyCap) {
        int np2 = 1;
        while (np2 < cnt) np2 <<= 1;
        if (cnt <= kAssocThreads) {
          // rank sort: key i lands at the number of smaller keys (unique:
          // the flat index is in the low bits); every thread reads the same
          // key at once (an LDS broadcast) -- cnt reads and two barriers
          // instead of log2(np2)^2 / 2 bitonic stages
          const uint64_t mine = tid < cnt ? keys[tid] : ~0ull;
          int r = 0;
          for (int j = 0; j < cnt; ++j) r += keys[j] < mine ? 1 : 0;
          __syncthreads();
          if (tid < cnt) keys[r] = mine;
          __syncthreads();
          np2 = 0;  // sorted
        }
        for (int i = cnt + tid; i < np2; i += kAssocThreads) keys[i] = ~0ull;
        __syncthreads();
        for (int size = 2; size <= np2; size <<= 1)
          for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < np2 / 2; i += kAssocThreads) {
              const int lo = 2 * i - (i & (stride - 1));
              const int hi = lo + stride;
              const bool up = (lo & size) == 0;
              const uint64_t a = keys[lo], c = keys[hi];
              if ((a > c) == up) {
                keys[lo] = c;
                keys[hi] = a;
              }
            }
            __syncthreads();
          }
        RV_PH(2);  // sort
        // greedy walk in (IoU desc, flat index asc) order, 64 pairs at a time:
        // a pair is accepted iff its row and column are still free; inside a
        // chunk the lowest remaining lane is accepted and the lanes sharing its
        // row or column are dropped (wave-uniform ballot loop)
        if (tid < 64) {
          for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            int t = -1, d = -2;
            bool ok = false;
            if (i < cnt) {
              const int f = (int)(keys[i] & 0xFFFFFFFFu);
              t = f / D;
              d = f - t * D;
              ok = trk_match[t] < 0 && det_match[d] < 0;
            }
            unsigned long long m = __ballot(ok);
            while (m) {
              const int q = __ffsll((long long)m) - 1;
              const int tq = __shfl(t, q), dq = __shfl(d, q);
              if (lane == q) {
                trk_match[t] = d;
                det_match[d] = t;
              }
              m &= ~__ballot(t == tq || d == dq);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
        }
      } else {
        // more qualifying pairs than keys: the literal reference loop (argmax
        // with the first maximum, accept, mask row and column) over M in HBM
        float* M = ws.M + (size_t)s * p.tmax * p.dmax;
        for (int i = tid; i < T * D; i += kAssocThreads) {
          const int t = i / D, d = i - (i / D) * D;
          // BYTE: a pair outside the stage is -1, as a masked row or column
          M[i] = in_stage(t, d) ? iou_f32(tbox[t], dbox[d]) : -1.0f;
        }
        __syncthreads();
        for (;;) {
          float bv = -INFINITY;
          int bi = 0x7FFFFFFF;
          for (int i = tid; i < T * D; i += kAssocThreads) {
            const float v = M[i];
            if (v > bv || (v == bv && i < bi)) {
              bv = v;
              bi = i;
            }
          }
          for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > bv || (ov == bv && oi < bi)) {
              bv = ov;
              bi = oi;
            }
          }
          if (lane == 0) {
            s_red_v[tid >> 6] = __float_as_int(bv);
            s_red_i[tid >> 6] = bi;
          }
          __syncthreads();
          bv = __int_as_float(s_red_v[0]);
          bi = s_red_i[0];
          for (int w = 1; w < kAssocThreads / 64; ++w) {
            const float ov = __int_as_float(s_red_v[w]);
            if (ov > bv || (ov == bv && s_red_i[w] < bi)) {
              bv = ov;
              bi = s_red_i[w];
            }
          }
          __syncthreads();
          if ((double)bv < thr) break;
          const int t = bi / D, d = bi - (bi / D) * D;
          if (tid == 0) {
            trk_match[t] = d;
            det_match[d] = t;
          }
          for (int j = tid; j < D; j += kAssocThreads) M[t * D + j] = -1.0f;
          for (int i = tid; i < T; i += kAssocThreads) M[i * D + d] = -1.0f;
          __syncthreads();
        }
      }
    }
