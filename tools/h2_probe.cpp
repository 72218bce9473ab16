// Stand-alone probe of the native h2 transport (ops/csrc/h2grpc_impl.h): an
// in-process H2Server on a unix socket, driven through H2GrpcClient::invoke_raw
// from T threads with B-call batches.  Every response is checked.  Prints
// calls/s, user and sys CPU microseconds per call and voluntary context
// switches per call (getrusage, client + server threads together), the
// slowest single batch and the transport counters.  It never initialises
// Python; the Python/pybind11 paths are needed only because the header
// carries the bindings' types.
//
//   g++ -std=c++17 -O2 -g -pthread tools/h2_probe.cpp -Iggrmcp_amd/ops/csrc \
//       $(python3 -m pybind11 --includes) -I/opt/conda/include \
//       -l:libnghttp2.so.14 $(python3-config --embed --ldflags) -o /tmp/h2_probe
//   /tmp/h2_probe --threads 4 --batch 61 --payload 1024 --conns 8 --seconds 3
//
// The same source is the sanitizer target: add
// -fsanitize=address,undefined -fno-omit-frame-pointer (or -fsanitize=thread)
// and run e.g.
//   /tmp/h2_probe --seconds 1 --backpressure --mute
// --backpressure sends 32 x 300 KB echoes down one connection (partial
// writes, POLLOUT); --mute sends a 16-call batch to a listener that never
// speaks h2 (every slot must come back DEADLINE_EXCEEDED, and closing the
// client afterwards must not hang).
//
// -DH2_GATHER_CAP=... / -DH2_DIRECT_SEND_MIN=... override the flush constants
// for A/B builds; GGRMCP_H2_RUN sets the placement run length at run time.

#include <sys/resource.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "h2grpc_impl.h"

static const char kHello[] = "/hello.HelloService/SayHello";
static const char kEcho[] = "/bench.EchoService/Echo";

static void put_varint(std::string& s, uint64_t v) {
  while (v >= 0x80) { s.push_back((char)(v | 0x80)); v >>= 7; }
  s.push_back((char)v);
}

// protobuf message with one length-delimited field 1 holding `body`
static std::string field1(const std::string& body) {
  std::string s;
  s.push_back('\x0a');
  put_varint(s, body.size());
  s += body;
  return s;
}

// the 5-byte gRPC prefix + message the transport hands back for `pb`
static std::string framed(const std::string& pb) {
  std::string s(5, '\0');
  uint32_t be = htonl((uint32_t)pb.size());
  memcpy(&s[1], &be, 4);
  return s + pb;
}

static double tv(const timeval& t) { return t.tv_sec * 1e6 + t.tv_usec; }

struct ThreadResult {
  uint64_t calls = 0, bad = 0;
  double slowest_ms = 0;
};

static void drive(H2GrpcClient* cli, int tid, int batch, size_t payload,
                  double seconds, ThreadResult* res) {
  std::vector<std::string> reqs(batch), want(batch);
  std::vector<H2GrpcClient::RawCall> rc(batch);
  auto t_end = Clock::now() + std::chrono::duration_cast<Clock::duration>(
                                  std::chrono::duration<double>(seconds));
  for (uint64_t b = 0; Clock::now() < t_end; ++b) {
    for (int i = 0; i < batch; ++i) {
      // distinct name per call: a response that belongs to another call
      // cannot pass the check
      char tag[48];
      int tl = snprintf(tag, sizeof(tag), "t%d.b%llu.i%d.", tid,
                        (unsigned long long)b, i);
      std::string name(tag, tl);
      if (name.size() < payload) name.append(payload - name.size(), 'x');
      reqs[i] = field1(name);
      want[i] = framed(field1("Hello, " + name + "!"));
      rc[i] = H2GrpcClient::RawCall{kHello, sizeof(kHello) - 1,
                                    (const uint8_t*)reqs[i].data(),
                                    reqs[i].size(), nullptr};
    }
    auto t0 = Clock::now();
    auto out = cli->invoke_raw(rc, 30.0);
    double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    res->slowest_ms = std::max(res->slowest_ms, ms);
    for (int i = 0; i < batch; ++i) {
      ++res->calls;
      if (std::get<0>(out[i]) != 0 || std::get<1>(out[i]) != want[i]) ++res->bad;
    }
  }
}

#ifdef GGRMCP_H2_STATS
static void print_stats(const char* who,
                        const std::unordered_map<std::string, uint64_t>& m) {
  std::vector<std::pair<std::string, uint64_t>> v(m.begin(), m.end());
  std::sort(v.begin(), v.end());
  printf("%s:", who);
  for (auto& kv : v) printf(" %s=%llu", kv.first.c_str(), (unsigned long long)kv.second);
  printf("\n");
}
#endif

// 32 calls of 300 KB on one connection: ~10 MB through a 4 MB socket buffer
static int run_backpressure(const std::string& target) {
  H2GrpcClient cli(target, 1, "localhost");
  const int n = 32;
  std::vector<std::string> reqs(n);
  std::vector<H2GrpcClient::RawCall> rc(n);
  for (int i = 0; i < n; ++i) {
    std::string body(300 * 1024, (char)('a' + i % 26));
    body[0] = (char)('A' + i % 26);
    reqs[i] = field1(body);
    rc[i] = H2GrpcClient::RawCall{kEcho, sizeof(kEcho) - 1,
                                  (const uint8_t*)reqs[i].data(), reqs[i].size(),
                                  nullptr};
  }
  auto out = cli.invoke_raw(rc, 30.0);
  int bad = 0;
  for (int i = 0; i < n; ++i)
    if (std::get<0>(out[i]) != 0 || std::get<1>(out[i]) != framed(reqs[i])) ++bad;
  printf("backpressure: %d calls of 300 KB on one connection, %d bad\n", n, bad);
#ifdef GGRMCP_H2_STATS
  print_stats("backpressure client", cli.stats());
#endif
  return bad;
}

// a listener that accepts and never speaks h2: nothing ever completes
static int run_mute() {
  int lfd = socket(AF_INET, SOCK_STREAM, 0);
  sockaddr_in addr{};
  addr.sin_family = AF_INET;
  inet_pton(AF_INET, "127.0.0.1", &addr.sin_addr);
  if (bind(lfd, (sockaddr*)&addr, sizeof(addr)) != 0 || listen(lfd, 8) != 0) {
    perror("mute listener");
    return 1;
  }
  socklen_t alen = sizeof(addr);
  getsockname(lfd, (sockaddr*)&addr, &alen);
  std::string target = "127.0.0.1:" + std::to_string(ntohs(addr.sin_port));
  int bad = 0;
  double waited = 0, closed = 0;
  {
    H2GrpcClient cli(target, 1, "localhost");
    int cfd = accept(lfd, nullptr, nullptr);
    const int n = 16;
    std::string req = field1("mute");
    std::vector<H2GrpcClient::RawCall> rc(
        n, H2GrpcClient::RawCall{kHello, sizeof(kHello) - 1,
                                 (const uint8_t*)req.data(), req.size(), nullptr});
    auto t0 = Clock::now();
    auto out = cli.invoke_raw(rc, 0.3);
    waited = std::chrono::duration<double>(Clock::now() - t0).count();
    for (int i = 0; i < n; ++i)
      if (std::get<0>(out[i]) != 4) ++bad;
    t0 = Clock::now();
    cli.close_all();
    closed = std::chrono::duration<double>(Clock::now() - t0).count();
    if (cfd >= 0) close(cfd);
  }
  close(lfd);
  if (waited > 0.3 + 2.0 + 1.0 || closed > 1.0) ++bad;
  printf("mute: 16 calls, timeout 0.3 s: returned after %.2f s, close took "
         "%.2f s, %d bad\n", waited, closed, bad);
  return bad;
}

int main(int argc, char** argv) {
  int threads = 4, batch = 61, conns = 8;
  size_t payload = 1024;
  double seconds = 3.0;
  bool backpressure = false, mute = false;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto val = [&]() -> const char* { return i + 1 < argc ? argv[++i] : "0"; };
    if (a == "--threads") threads = atoi(val());
    else if (a == "--batch") batch = atoi(val());
    else if (a == "--conns") conns = atoi(val());
    else if (a == "--payload") payload = (size_t)atol(val());
    else if (a == "--seconds") seconds = atof(val());
    else if (a == "--backpressure") backpressure = true;
    else if (a == "--mute") mute = true;
    else {
      fprintf(stderr, "usage: %s [--threads T] [--batch B] [--payload BYTES] "
              "[--conns C] [--seconds S] [--backpressure] [--mute]\n", argv[0]);
      return 2;
    }
  }
  std::string target = "unix:/tmp/h2_probe." + std::to_string(getpid()) + ".sock";
  H2Server srv(target);
  srv.add_route(kHello, "hello");
  srv.add_route(kEcho, "echo");
  srv.start();
  int bad = 0;
  {
    H2GrpcClient cli(target, conns, "localhost");
    ThreadResult warm;
    drive(&cli, 99, batch, payload, 0.2, &warm);  // SETTINGS, HPACK tables
    bad += (int)warm.bad;

    std::vector<ThreadResult> res(threads);
    std::vector<std::thread> ts;
    rusage r0{}, r1{};
    getrusage(RUSAGE_SELF, &r0);
    auto t0 = Clock::now();
    for (int t = 0; t < threads; ++t)
      ts.emplace_back(drive, &cli, t, batch, payload, seconds, &res[t]);
    for (auto& t : ts) t.join();
    double wall = std::chrono::duration<double>(Clock::now() - t0).count();
    getrusage(RUSAGE_SELF, &r1);

    uint64_t calls = 0;
    double slowest = 0;
    for (auto& r : res) {
      calls += r.calls;
      bad += (int)r.bad;
      slowest = std::max(slowest, r.slowest_ms);
    }
    double user = tv(r1.ru_utime) - tv(r0.ru_utime);
    double sys = tv(r1.ru_stime) - tv(r0.ru_stime);
    printf("T=%d B=%d payload=%zu conns=%d: %.0f calls/s, cpu %.2f us/call "
           "(user %.2f, sys %.2f), %.3f vol ctx switches/call, slowest batch "
           "%.2f ms, %llu calls, %d bad\n",
           threads, batch, payload, conns, calls / wall, (user + sys) / calls,
           user / calls, sys / calls,
           (double)(r1.ru_nvcsw - r0.ru_nvcsw) / calls, slowest,
           (unsigned long long)calls, bad);
#ifdef GGRMCP_H2_STATS
    print_stats("client", cli.stats());
    print_stats("server", srv.stats());
#endif
  }
  if (backpressure) bad += run_backpressure(target);
  if (mute) bad += run_mute();
  srv.stop();
  unlink(target.c_str() + 5);
  return bad ? 1 : 0;
}
