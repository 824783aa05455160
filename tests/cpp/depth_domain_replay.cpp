// TEST INFRASTRUCTURE (never part of the product path): the frames of tests/depth_domain_frames.py -- float depth that no millimetre image
// holds: NaN, infinities, negative, denormal, far and off-grid values -- replayed through the oracle's entry points the GPU tests compare
// against, in a program of its own, so that tests/test_depth_domain_oracle.py can build it with the address and undefined-behaviour sanitizers
// and run it as a child process.  A clean end is what makes the oracle a reference on a class of values at a stage; a report takes that
// class out of that stage's table (STAGE_EXCLUDES).
//
//   depth_domain_replay FILE STAGE...      FILE as depth_domain_frames.write_replay_file lays it out; every sequence goes through every stage
//     sdf, ofusion   so_pipe_integrate + so_pipe_raycast of every frame (mu 0.1 / 0.02), then the whole map read back
//     pyramid        so_half_sample twice (e_d = 3 e_delta, r = 1, as DenseSLAMSystem::tracking builds scaled_depth_) of every frame
//     filter         so_bilateral_filter of every frame
//     track          SDF: frames 0 .. n-2 fused and raycast, frame n-1 tracked from pose n-2 on a (4, 3, 2) pyramid, plain and filtered
//     render         so_render_depth of every frame
//   One line per sequence and stage on stdout: name, stage, then key / value pairs.
#include "../../oracle/se_oracle.cpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

struct Sequence {
  char name[33];
  int W, H, N, frames;
  float dim, k[4];
  std::vector<std::vector<float>> pose, depth;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

bool read_file(const char* path, std::vector<Sequence>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  int32_t count = 0;
  bool ok = read_exact(f, &count, 4) && count >= 0 && count < 4096;
  for (int s = 0; ok && s < count; ++s) {
    Sequence q;
    int32_t hdr[4];
    float fl[5];
    ok = read_exact(f, q.name, 32) && read_exact(f, hdr, sizeof hdr) && read_exact(f, fl, sizeof fl);
    if (!ok) break;
    q.name[32] = 0;
    q.W = hdr[0]; q.H = hdr[1]; q.N = hdr[2]; q.frames = hdr[3];
    q.dim = fl[0];
    for (int i = 0; i < 4; ++i) q.k[i] = fl[1 + i];
    ok = q.W > 0 && q.H > 0 && q.W <= 4096 && q.H <= 4096 && q.N >= 64 && q.N <= 4096 && q.frames > 0 && q.frames <= 64;
    for (int i = 0; ok && i < q.frames; ++i) {
      q.pose.emplace_back(16);
      q.depth.emplace_back((size_t)q.W * q.H);
      ok = read_exact(f, q.pose.back().data(), 64) && read_exact(f, q.depth.back().data(), q.depth.back().size() * 4);
    }
    if (ok) out.push_back(std::move(q));
  }
  std::fclose(f);
  return ok;
}

size_t count_nan(const std::vector<float>& v) {
  size_t n = 0;
  for (float x : v) n += std::isnan(x) ? 1 : 0;
  return n;
}

// integrate + raycast frames [0, upto); returns the pipeline, the last raycast in vertex / normal
void* fuse(const Sequence& q, int field, float mu, int upto, std::vector<float>& vertex, std::vector<float>& normal, uint64_t* oob_ub_integration, int* last_raycast) {
  void* p = so_pipe_create(field, q.N, q.dim, q.W, q.H);
  so_pipe_count_stats(p, 1);
  vertex.assign((size_t)q.W * q.H * 3, 0.f);
  normal.assign((size_t)q.W * q.H * 3, 0.f);
  uint64_t st[11];
  *oob_ub_integration = 0;
  *last_raycast = -1;
  for (int f = 0; f < upto; ++f) {
    so_pipe_stats(p, st);
    const uint64_t before = st[10];
    so_pipe_integrate(p, q.depth[f].data(), q.pose[f].data(), q.k, 1, mu, (unsigned)f);
    so_pipe_stats(p, st);
    *oob_ub_integration += st[10] - before;
    if (so_pipe_raycast(p, q.pose[f].data(), q.k, mu, (unsigned)f, vertex.data(), normal.data())) *last_raycast = f;
  }
  return p;
}

void stage_field(const Sequence& q, const char* stage, int field, float mu) {
  std::vector<float> vertex, normal;
  uint64_t oob_ub = 0;
  int last = -1;
  void* p = fuse(q, field, mu, q.frames, vertex, normal, &oob_ub, &last);
  int nb = 0, nn = 0;
  so_pipe_counts(p, &nb, &nn);
  std::vector<int32_t> coords((size_t)nb * 3);
  std::vector<float> x((size_t)nb * 512), y((size_t)nb * 512), nx((size_t)nn * 8), ny((size_t)nn * 8);
  std::vector<uint8_t> active(nb);
  std::vector<uint64_t> code(nn);
  std::vector<uint32_t> side(nn);
  if (nb) so_pipe_get_blocks(p, coords.data(), x.data(), y.data(), active.data());
  so_pipe_get_nodes(p, code.data(), side.data(), nx.data(), ny.data());
  uint64_t st[11];
  so_pipe_stats(p, st);
  size_t hits = 0;
  for (size_t i = 0; i < normal.size(); i += 3) hits += normal[i] != INVALID ? 1 : 0;
  std::printf("%s %s blocks %d nodes %d nan %zu hits %zu probes %llu truncated %llu oob_ub_integration %llu raycast %d\n", q.name, stage, nb, nn,
              count_nan(x) + count_nan(y) + count_nan(nx) + count_nan(ny), last >= 0 ? hits : (size_t)0, (unsigned long long)st[0],
              (unsigned long long)st[9], (unsigned long long)oob_ub, last);
  so_pipe_destroy(p);
}

void stage_pyramid(const Sequence& q) {
  size_t nan1 = 0, nan2 = 0;
  for (int f = 0; f < q.frames; ++f) {
    const int w1 = q.W / 2, h1 = q.H / 2, w2 = w1 / 2, h2 = h1 / 2;
    std::vector<float> l1((size_t)w1 * h1), l2((size_t)w2 * h2);
    so_half_sample(l1.data(), w1, h1, q.depth[f].data(), q.W, e_delta * 3, 1);
    so_half_sample(l2.data(), w2, h2, l1.data(), w1, e_delta * 3, 1);
    nan1 += count_nan(l1);
    nan2 += count_nan(l2);
  }
  std::printf("%s pyramid nan1 %zu nan2 %zu\n", q.name, nan1, nan2);
}

void stage_filter(const Sequence& q) {
  size_t nans = 0;
  for (int f = 0; f < q.frames; ++f) {
    std::vector<float> out((size_t)q.W * q.H);
    so_bilateral_filter(out.data(), q.depth[f].data(), q.W, q.H);
    nans += count_nan(out);
  }
  std::printf("%s filter nan %zu\n", q.name, nans);
}

void stage_track(const Sequence& q) {
  if (q.frames < 2) return;
  std::vector<float> vertex, normal;
  uint64_t oob_ub = 0;
  int last = -1;
  void* p = fuse(q, 0, 0.1f, q.frames - 1, vertex, normal, &oob_ub, &last);
  if (last < 0) { std::printf("%s track no-raycast\n", q.name); so_pipe_destroy(p); return; }
  const int iterations[3] = {4, 3, 2};
  const std::vector<float>& depth = q.depth[q.frames - 1];
  std::vector<float> filtered(depth.size());
  so_bilateral_filter(filtered.data(), depth.data(), q.W, q.H);
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<float> pose = q.pose[q.frames - 2];
    std::vector<unsigned char> track((size_t)q.W * q.H * 32);
    float reduce[32];
    int iters = 0;
    const int ok = so_tracking(pass ? filtered.data() : depth.data(), q.W, q.H, q.k, iterations, 3, 1e-5f, vertex.data(), normal.data(), q.pose[last].data(),
                               pose.data(), track.data(), reduce, &iters);
    std::printf("%s track%s tracked %d iterations %d inliers %.0f\n", q.name, pass ? "-filtered" : "", ok, iters, reduce[28]);
  }
  so_pipe_destroy(p);
}

void stage_render(const Sequence& q) {
  unsigned long long sum = 0;
  for (int f = 0; f < q.frames; ++f) {
    std::vector<unsigned char> out((size_t)q.W * q.H * 4);
    so_render_depth(out.data(), q.depth[f].data(), q.W, q.H);
    for (unsigned char c : out) sum += c;
  }
  std::printf("%s render bytes-sum %llu\n", q.name, sum);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s FILE STAGE...\n", argv[0]); return 2; }
  std::vector<Sequence> seqs;
  if (!read_file(argv[1], seqs)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  for (const Sequence& q : seqs)
    for (int a = 2; a < argc; ++a) {
      const std::string s = argv[a];
      if (s == "sdf") stage_field(q, "sdf", 0, 0.1f);
      else if (s == "ofusion") stage_field(q, "ofusion", 1, 0.02f);
      else if (s == "pyramid") stage_pyramid(q);
      else if (s == "filter") stage_filter(q);
      else if (s == "track") stage_track(q);
      else if (s == "render") stage_render(q);
      else { std::fprintf(stderr, "unknown stage %s\n", s.c_str()); return 2; }
      std::fflush(stdout);
    }
  return 0;
}
