// Runs of a ragged row table (row_seq[r], row_pos[r]): a run is a maximal stretch of consecutive rows of one sequence whose
// positions rise by exactly one.  One definition for the launches that read the table: mq_decode_attention_ragged (csrc/mq_decode_rows.hip)
// and mq_sample_ragged (csrc/mq_sample.hip).
#pragma once

namespace mq {

// Rows of row r's run in front of it, at most max_front: r is live, sb = row_seq[r] and pos = row_pos[r] are range-checked by the caller.
// A row in front belongs to the run iff it names sb at the position one below its successor's, so every row counted is live as well
// (its position lies in [0, pos)) and only entries below r are read.  r is the workgroup's row: the loads are wave-uniform (scalar).
__device__ __forceinline__ int run_rows_in_front(const int* row_seq, const int* row_pos, int r, int sb, int pos, int max_front) {
  int j = 0;
  while (j < r && j < max_front && pos - 1 - j >= 0 && row_seq[r - 1 - j] == sb && row_pos[r - 1 - j] == pos - 1 - j) ++j;
  return j;
}

}  // namespace mq
