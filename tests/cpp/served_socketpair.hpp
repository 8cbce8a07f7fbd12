// served_socketpair.hpp -- TEST INFRASTRUCTURE ONLY.
//
// A srpc::gpu::batch_server serving one end of a socketpair on a thread; the
// test talks to `fd`.  Shared by gpu_server_ordered_test.cpp,
// gpu_server_ordered_var_test.cpp, gpu_records_test.cpp and
// gpu_server_routes_test.cpp.
#pragma once

#include <srpc/gpu_server.hpp>
#include <sys/socket.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>

struct served_socketpair {
    int fd = -1, sfd = -1;
    std::thread t;
    srpc::gpu::batch_stats stats;
    int thrown = 0;  // the plan_error serve_connection ended with, 0: none

    /// A server of its own: built on the thread, `setup` registers its methods.
    served_socketpair(uint64_t max_batch, std::function<void(srpc::gpu::batch_server&)> setup,
                      srpc::server* fallback = nullptr) {
        open();
        t = std::thread([this, max_batch, setup, fallback] {
            srpc::gpu::batch_server srv(max_batch, 0, fallback);
            setup(srv);
            serve(srv);
        });
    }
    /// One connection of a server the test keeps (and serves again later).
    explicit served_socketpair(srpc::gpu::batch_server& srv) {
        open();
        t = std::thread([this, &srv] { serve(srv); });
    }
    void finish() {
        shutdown(fd, SHUT_WR);
        t.join();
        close(fd);
    }

private:
    void open() {
        int sv[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
        fd = sv[0];
        sfd = sv[1];
    }
    void serve(srpc::gpu::batch_server& srv) {
        try {
            stats = srv.serve_connection(sfd);
        } catch (srpc::gpu::plan_error const& e) {
            thrown = e.code;
            std::fprintf(stderr, "server: %s\n", e.what());
        }
        close(sfd);
    }
};
