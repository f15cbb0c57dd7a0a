// tools/wav_fuzz.cpp -- the header readers of csrc/qvc_io.cpp over a directory of damaged files, as a stand-alone program
// for a sanitizer build (host code only; nothing here touches a GPU or Python):
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import wavgen; \
//              [open(f'{sys.argv[1]}/d{i:03d}.wav', 'wb').write(b) for i, b in enumerate(wavgen.damaged_corpus())]" DIR
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread \
//       tools/wav_fuzz.cpp quickvc-official_amd/csrc/qvc_io.cpp -o wav_fuzz && ./wav_fuzz DIR
//
// The corpus is the one tests/test_wav_io_host.py uses (a valid header cut at every length and with random bytes
// overwritten).  Every file goes through qvc_io_wav_headers, qvc_io_load_wavs (slots of 64 bytes between two guard
// blocks that must not change) and qvc_io_npy_shape; the program adds two .npy headers of its own, one of them with only
// spaces after 'fortran_order':.  Exit status 0 = every call returned a status and no guard byte changed.
#include "../include/qvc_io.h"

#include <dirent.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

static bool write_npy(const std::string& path, const char* dict) {
  std::string h(dict);
  h.resize(118, ' ');
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const unsigned char pre[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, 118, 0};
  std::fwrite(pre, 1, 10, f);
  std::fwrite(h.data(), 1, h.size(), f);
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  if (!write_npy(dir + "/spaces.npy", "{'descr': '<f4', 'shape': (3, 256), 'fortran_order':") ||
      !write_npy(dir + "/good.npy", "{'descr': '<f4', 'fortran_order': False, 'shape': (3, 256), }")) return 2;
  std::vector<std::string> names;
  DIR* d = opendir(dir.c_str());
  if (!d) { std::perror("opendir"); return 2; }
  while (dirent* e = readdir(d))
    if (e->d_name[0] != '.') names.push_back(dir + "/" + e->d_name);
  closedir(d);
  names.push_back(dir + "/no-such-file.wav");
  const int32_t n = (int32_t)names.size();
  std::vector<const char*> paths;
  for (auto& s : names) paths.push_back(s.c_str());

  qvc_io_pool* pool = nullptr;
  if (qvc_io_pool_create(4, &pool) != QVC_IO_OK) return 2;
  std::vector<qvc_wav_header> hdr((size_t)n);
  std::vector<int32_t> st((size_t)n, 99), st2((size_t)n, 99);
  const int rc = qvc_io_wav_headers(pool, paths.data(), n, hdr.data(), st.data());
  const int64_t slot = 64, guard = 4096;
  std::vector<uint8_t> buf((size_t)(2 * guard + n * slot), 0xA5);
  const int rc2 = qvc_io_load_wavs(pool, paths.data(), n, buf.data() + guard, slot, nullptr, st2.data());
  std::map<int, int> seen, seen2, seen3;
  int bad = 0;
  for (int32_t i = 0; i < n; ++i) {
    ++seen[st[(size_t)i]]; ++seen2[st2[(size_t)i]];
    if (st[(size_t)i] > 0 || st[(size_t)i] < QVC_IO_ERR_IO || st2[(size_t)i] > 0 || st2[(size_t)i] < QVC_IO_ERR_IO) ++bad;
    int32_t fr = 0, co = 0;
    ++seen3[qvc_io_npy_shape(paths[(size_t)i], &fr, &co)];
  }
  for (int64_t i = 0; i < guard; ++i)
    if (buf[(size_t)i] != 0xA5 || buf[(size_t)(guard + n * slot + i)] != 0xA5) { ++bad; break; }
  int32_t fr = 0, co = 0;
  const int spaces = qvc_io_npy_shape((dir + "/spaces.npy").c_str(), &fr, &co);
  const int good = qvc_io_npy_shape((dir + "/good.npy").c_str(), &fr, &co);
  if (spaces != QVC_IO_ERR_FORMAT || good != QVC_IO_OK || fr != 3 || co != 256) ++bad;
  qvc_io_pool_destroy(pool);
  std::printf("%d files: wav_headers -> %d, load_wavs -> %d\n", n, rc, rc2);
  for (auto& kv : seen) std::printf("  wav_headers status %d: %d files\n", kv.first, kv.second);
  for (auto& kv : seen2) std::printf("  load_wavs   status %d: %d files\n", kv.first, kv.second);
  for (auto& kv : seen3) std::printf("  npy_shape   status %d: %d files\n", kv.first, kv.second);
  std::printf("  npy 'fortran_order' followed by spaces only -> %d, a good header -> %d\n%s\n", spaces, good, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
